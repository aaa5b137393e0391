/*
 * ov2slam_hip.h -- C ABI of libov2slam_hip.so (MI355X / gfx950 HIP kernels).
 *
 * Drop-in boundary for OV2SLAM's front-end + local-BA hot path.  The reference
 * has no FFI layer: the boundary is three C++ classes (FeatureExtractor,
 * FeatureTracker, Optimizer) that call OpenCV / Ceres.  A thin C++ adapter with
 * the reference's own signatures (the headers in ov2slam_amd/host/)
 * forwards to the entry points below.  Plain pointers and sizes only; no
 * OpenCV / Eigen / torch types.  All citations are relative to /root/reference.
 *
 * Conventions
 *   - every function returns 0 (OV2_OK) on success, a negative OV2_E* otherwise,
 *     and never throws or aborts; on error no output buffer is modified unless
 *     stated (the adapter maps errors to the reference's "nothing tracked /
 *     BA skipped" behaviour, SURVEY.md 5 "failure detection").
 *   - `*_h` pointers are host memory, `*_d` pointers are device (HBM) memory.
 *   - an ov2_ctx owns one HIP stream + scratch; one ctx per calling thread
 *     (fbKltTracking is called concurrently from the SLAM and mapper threads,
 *     src/visual_front_end.cpp:196 vs src/map_manager.cpp:510).  The library is
 *     re-entrant across contexts.
 *   - keypoints are float2 (x,y) interleaved, like std::vector<cv::Point2f>.
 */
#ifndef OV2SLAM_HIP_H
#define OV2SLAM_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OV2_OK            0
#define OV2_EINVAL       -1   /* bad argument                                  */
#define OV2_EHIP         -2   /* HIP runtime error (see ov2_last_error)        */
#define OV2_ENOMEM       -3
#define OV2_EUNSUPPORTED -4   /* e.g. LK window size without a kernel instance */
#define OV2_ENODEVICE    -5   /* no gfx950 device visible                      */

typedef struct ov2_ctx ov2_ctx;
typedef struct ov2_pyr ov2_pyr;

/* ---- context ------------------------------------------------------- */
/* ABI version of THIS header: bumped whenever a struct passed by pointer grows or an entry point changes its signature
 * (round 2 added ov2_ba_options::max_solver_time_s).  ov2_version() returns the value the library was built with; a caller
 * must refuse to run when the two differ (the C++ adapters' ov2::Context and ov2slam_amd/_lib.py do): a shorter options
 * struct from an older header would otherwise be read past its end.                                                    */
#define OV2_ABI_VERSION 600
int  ov2_version(void);
/* last error message of the calling thread ("" if none); never NULL */
const char *ov2_last_error(void);
/* creates a context with its own non-blocking HIP stream on `device` */
int  ov2_ctx_create(int device, ov2_ctx **out);
/* same with a stream priority: > 0 the device's highest, < 0 its lowest, 0 = ov2_ctx_create.  A host that runs several contexts on one
 * GPU states what is latency-critical: the reference's SLAM thread is real time while its estimator thread works on whatever
 * keyframe is newest when it gets round to it (src/estimator.cpp:195-205) -- tools/lockstep_driver.cpp gives the tracking context the
 * high priority and the localBA contexts the low one, so that a dozen concurrent solves do not stretch the per-frame enqueue */
int  ov2_ctx_create_with_priority(int device, int priority, ov2_ctx **out);
/* same, but enqueue on an existing hipStream_t (e.g. torch's current stream) */
int  ov2_ctx_create_on_stream(int device, void *hip_stream, ov2_ctx **out);
void ov2_ctx_destroy(ov2_ctx *ctx);
int  ov2_ctx_sync(ov2_ctx *ctx);
void *ov2_ctx_stream(ov2_ctx *ctx);        /* the hipStream_t, for event timing */
/* Per-context options.
 * OV2_OPT_SOBEL_DY_ORDER: evaluation order of cv::Sobel(dx = 0, dy = 1, scale) inside cv::cornerMinEigenVal
 * (detectSingleScale, src/feature_extractor.cpp:354).  OpenCV multiplies the SMOOTHING kernel by the scale when dx == 0,
 * so its 8U -> 32F row pass rounds ((p[x-1] k0 + p[x] k1) + p[x+1] k2) per pixel and the column pass subtracts two
 * rounded rows: OV2_SOBEL_DY_OPENCV_ROWFILTER, the default.  OV2_SOBEL_DY_EXACT_SUM scales the exact integer difference
 * instead (<= 1 ulp apart per pixel; can flip arg-max ties).  Neither is pinned against a real OpenCV build.           */
#define OV2_OPT_SOBEL_DY_ORDER         1
#define OV2_SOBEL_DY_OPENCV_ROWFILTER  0
#define OV2_SOBEL_DY_EXACT_SUM         1
/* Path selection.  Every kernel choice the library makes by itself can be pinned per context -- the parity tests run every
 * path on the same inputs this way, A/B measurements use it.  The library reads no environment variable after ov2_ctx_create
 * (its entry points are called from several threads of a host process that may call setenv concurrently).
 * OV2_OPT_LK_IMPL           ov2_fb_klt* / ov2_lk_track with the reference's window (9): AUTO picks the 3-lanes-per-keypoint kernel
 *                           (lk3.hip) from 65536 points per call on, the row-per-lane kernel (lk.hip) below
 * OV2_OPT_LK_PERSIST        the 3-lanes-per-keypoint kernel's launch form.  -1 (default): launches of more keypoint blocks than the device
 *                           holds work-groups at once run persistent -- a small kernel lists the (item, block) pairs that hold a
 *                           keypoint, and one round of resident work-groups pulls them until none is left; smaller launches keep
 *                           one work-group per block.  0: always one work-group per block.  N > 0: always persistent, with exactly N
 *                           work-groups (tests, A/B measurements).  Results do not depend on it
 *                           The unit lists live in a buffer of the context that grows (is freed and allocated again) when a
 *                           launch needs more room than any before it.  A captured graph keeps the pointer it was captured with:
 *                           make the largest launch once BEFORE capturing, as for every grow-only buffer of a context
 * OV2_OPT_TRACK_IMPL        ov2_tracker_* / ov2_stereo_match, window 9: wavefront per keypoint (lkw.hip, default) or row per lane
 * OV2_OPT_CLAHE_STRIPS      ov2_pyr_build_clahe_*: the one-walk strip kernel (CLAHE apply + level 1 + borders): -1 auto (batch x
 *                           strips >= 1024: the fused form), 0 never, 1 whenever the geometry allows, after the LUT kernel,
 *                           2 whenever the geometry allows, fused with the LUT computation (one launch, LUTs stay in LDS)
 * OV2_OPT_BA_FORCE_LARGE    1: the large-problem BA path (sparse W slots, HBM Cholesky) on a problem of any size
 * OV2_OPT_BA_LIN_DIRECT     1 (with FORCE_LARGE): the lineariser without LDS aggregation of the observer blocks
 * OV2_OPT_BA_SCHUR_CHUNK    columns of the sparse Schur row block kept in LDS per chunk (0 = auto)
 * OV2_OPT_BA_XYZ_LIN_WAVES  wavefronts per work-group of the 3-D-point lineariser: 0 auto, 1, 2
 * OV2_OPT_BA_POSE_ONLY_FUSED 0: ceresPnP through the multi-kernel LM loop instead of the one-kernel form (default 1)
 * OV2_OPT_BA_DETERMINISTIC 1: bit-identical results from run to run (the reference solves with num_threads = 1): every sum that the
 *                           default accumulates with fp64 atomics in arrival order (H, F^T b, W^T C W, the costs) goes through
 *                           per-work-group buffers added up in a fixed order.  Inverse-depth form on the LDS-resident path (up
 *                           to ~70 optimised keyframes); other forms answer OV2_EUNSUPPORTED while it is set.  ~1.7x the solve time.
 * OV2_OPT_FAST_TIE          detectGridFAST: which of several EQUAL best FAST responses of a cell wins.  The reference sorts the cell's corners
 *                           with std::sort (src/feature_extractor.cpp:518, not stable) and takes the first: with more than 16 corners left
 *                           the winner among ties is the standard library's choice.  OV2_FAST_TIE_LIBSTDCXX (default): libstdc++'s
 *                           introsort restated -- the reference as built with g++, cell for cell (tests/test_reference_factors.py runs
 *                           the reference's own source); OV2_FAST_TIE_SCAN_ORDER: the first in scan order (what a stable sort gives)
 * OV2_OPT_LK_ACC            accumulator type of calcOpticalFlowPyrLK's sums (normal matrix, mismatch vector).  OpenCV's LKTrackerInvoker
 *                           is written against `acctype`: int64 on ARM without NEON, FLOAT everywhere else (lkpyramid.cpp).
 *                           OV2_LK_ACC_INT64 (default): exact integer sums -- independent of summation order, the form every kernel
 *                           implements and the oracle's canonical mode.  OV2_LK_ACC_FLOAT_UI4: float accumulators in the order an x86
 *                           OpenCV 4.x build (128-bit universal intrinsics, no FMA) adds them -- what the reference executes at
 *                           src/feature_tracker.cpp:66-69 / :113-116 on a desktop; restated from the public source (oracle:
 *                           ORC_LK_ACC_FLOAT_UI4), bit-exact against that restatement, never checked against an OpenCV binary.
 *                           Applies to ov2_fb_klt* / ov2_lk_track (row-per-lane kernel, any window), ov2_tracker_* / ov2_btracker_* /
 *                           ov2_stereo_match* (both kernels); a tracker captures its graphs at creation: set the option before.
 *                           Measured on EuRoC-like frames: no status flips, positions within 1.5e-4 px of the INT64 mode.
 * OV2_OPT_DEBUG             1: timing laps of ov2_local_ba / detection on stderr (initial value: environment OV2_DEBUG at
 *                           ov2_ctx_create, the only environment variable the library ever reads)                          */
#define OV2_OPT_LK_IMPL            2
#define OV2_LK_IMPL_AUTO           0
#define OV2_LK_IMPL_ROW            1
#define OV2_LK_IMPL_LANE3          2
#define OV2_OPT_LK_PERSIST         17
#define OV2_OPT_TRACK_IMPL         3
#define OV2_TRACK_IMPL_WAVE        0
#define OV2_TRACK_IMPL_ROW         1
#define OV2_OPT_CLAHE_STRIPS       4
#define OV2_OPT_BA_FORCE_LARGE     5
#define OV2_OPT_BA_LIN_DIRECT      6
#define OV2_OPT_BA_SCHUR_CHUNK     7
#define OV2_OPT_BA_XYZ_LIN_WAVES   8
#define OV2_OPT_BA_POSE_ONLY_FUSED 9
#define OV2_OPT_BA_DETERMINISTIC   10
#define OV2_OPT_DEBUG              11
#define OV2_OPT_FAST_TIE           12
#define OV2_FAST_TIE_SCAN_ORDER    0
#define OV2_FAST_TIE_LIBSTDCXX     1
#define OV2_OPT_DETECT_STRIP       15   /* detectSingleScale's response kernel: -1 auto (the strip kernel for batches: the free cells of an image side by
                                           side, ~59 of 64 lanes busy on 35-pixel cells), 0 one wavefront per cell, 1 the strip kernel; same bits */
#define OV2_OPT_LK_ACC             14
#define OV2_LK_ACC_INT64           0
#define OV2_LK_ACC_FLOAT_UI4       1
#define OV2_OPT_BA_TRACE           13   /* 1: ov2_ba_solve / ov2_ba_solve_resident / ov2_xyz_ba_solve / each pass of ov2_local_ba record the
                                           iteration summaries of the solve (ov2_ba_get_trace); the batch entry point does not */
#define OV2_OPT_LCKF_SCRATCH_KB    16   /* ov2_lckf_prepare*: device scratch (KiB) the batch forms may hold at a time; items are walked in chunks
                                           that fit (at least one item per chunk).  Default 262144 (256 MiB); >= 1 */
#define OV2_OPT_EPIF_CAPACITY      18   /* test forcing: 1 makes ov2_epipolar_filter[_batch] stage its device block in the CAPACITY form (every item
                                           owns as many keypoint / keyframe slots as the largest item of the call), the form a fused step
                                           will use; the results do not depend on it.  Default 0: packed to the items' sizes */
int  ov2_ctx_set_option(ov2_ctx *ctx, int option, int value);
int  ov2_ctx_get_option(ov2_ctx *ctx, int option, int *value);

/* ---- image pyramid -------------------------------------------------
 * Replaces cv::buildOpticalFlowPyramid(img, pyr, Size(win,win), max_level)
 *   src/visual_front_end.cpp:1172, :53 ; src/mapper.cpp:81
 * (withDerivatives=true, pyrBorder=REFLECT_101, derivBorder=CONSTANT).
 * `batch` independent images of identical size are built in one launch set
 * (batch=1 is the drop-in case; batch>1 is the offline batch-of-sequences
 * mode of BASELINE.json config 5).  Image b starts at img + b*img_batch_stride.
 */
int  ov2_pyr_create(ov2_ctx *ctx, int w, int h, int win, int max_level, int batch, ov2_pyr **out);
void ov2_pyr_destroy(ov2_pyr *p);
int  ov2_pyr_levels(const ov2_pyr *p);                 /* levels actually built */
int  ov2_pyr_level_size(const ov2_pyr *p, int level, int *w, int *h);
int  ov2_pyr_batch(const ov2_pyr *p);
/* A batch-1 pyramid that ALIASES batch item `item` of `p` (no copy, no allocation on the device): what the entry points that
 * take batch-1 pyramids (ov2_stereo_match, ov2_fb_klt, ov2_detect_*_d ...) need to work on one sequence of a lock-step batch.
 * The view shares p's `ready` hand-off (a consumer on another context waits for p's last build) and must be destroyed
 * (ov2_pyr_destroy) before p.                                                                                        */
int  ov2_pyr_item_view(const ov2_pyr *p, int item, ov2_pyr **out);
/* (re)build from host images: H2D copy + kernels, asynchronous on ctx's stream.  A batch-1 image is repacked into the context's
 * pinned staging buffer before the call returns (one contiguous DMA whatever the row stride; the caller's buffer is free at
 * once); for batch > 1 the host buffer must stay valid until ov2_ctx_sync / a later blocking call */
int  ov2_pyr_build_h(ov2_ctx *ctx, ov2_pyr *p, const uint8_t *img_h, int stride, size_t img_batch_stride);
/* (re)build from images already resident in HBM */
int  ov2_pyr_build_d(ov2_ctx *ctx, ov2_pyr *p, const uint8_t *img_d, int stride, size_t img_batch_stride);
/* D2H of one level of batch item b: un-padded image (w*h u8) and/or derivative
 * (w*h int16x2); either pointer may be NULL.  Blocking.                        */
int  ov2_pyr_download(ov2_ctx *ctx, const ov2_pyr *p, int b, int level, uint8_t *img_h, int16_t *deriv_h);
/* same but including the `win` border on every side ((w+2win)*(h+2win))        */
int  ov2_pyr_download_padded(ov2_ctx *ctx, const ov2_pyr *p, int b, int level, uint8_t *img_h, int16_t *deriv_h);
/* algorithmic HBM bytes of one build of one image (SURVEY.md 8d "B_pyr")       */
size_t ov2_pyr_algorithmic_bytes(const ov2_pyr *p);
/* One batch item as it lies in device memory: every level with its borders and the alignment slack between them,
 * ov2_pyr_item_bytes(p) bytes (the stride between items).  For comparing pyramids byte by byte (tests). */
size_t ov2_pyr_item_bytes(const ov2_pyr *p);
int  ov2_pyr_download_item(ov2_ctx *ctx, const ov2_pyr *p, int b, uint8_t *bytes_h);

/* ---- CLAHE ----------------------------------------------------------
 * Replaces cv::CLAHE::apply(img_raw, cur_img_) -- src/visual_front_end.cpp:1159 (left image, every
 * frame when use_clahe: 1), src/mapper.cpp:76 (right image) -- for the handle created at
 * src/ov2slam.cpp:85-89: cv::createCLAHE(clip_limit = fclahe_val, tiles = (w/50, h/50)).
 * CV_8UC1 only (what the reference feeds it).  _h: host buffers (drop-in); _d: `batch` images
 * already in HBM, src and dst must not overlap. */
int ov2_clahe_h(ov2_ctx *ctx, const uint8_t *src_h, int w, int h, int stride, double clip_limit, int tiles_x, int tiles_y,
                uint8_t *dst_h, int dst_stride);
int ov2_clahe_d(ov2_ctx *ctx, const uint8_t *src_d, int w, int h, int stride, size_t src_batch_stride, int batch,
                double clip_limit, int tiles_x, int tiles_y, uint8_t *dst_d, int dst_stride, size_t dst_batch_stride);
/* preprocessImage in one call: CLAHE of img_d written straight into the pyramid's level 0, then the
 * coarser levels -- the pair clahe->apply(img_raw, cur_img_) + cv::buildOpticalFlowPyramid(cur_img_, ...)
 * of src/visual_front_end.cpp:1159 + :1172 (mapper.cpp:76 + :81) without the intermediate image.
 * Results are identical to ov2_clahe_d followed by ov2_pyr_build_d; the equalised image stays
 * available as level 0 of the pyramid.                                                            */
int ov2_pyr_build_clahe_d(ov2_ctx *ctx, ov2_pyr *p, const uint8_t *img_d, int stride, size_t img_batch_stride,
                          double clip_limit, int tiles_x, int tiles_y);
/* same from a host image (batch-1 pyramid): one H2D of the raw frame, asynchronous on ctx's stream -- the
 * single-sequence form of VisualFrontEnd::preprocessImage (the image is staged in pinned memory before the call returns) */
int ov2_pyr_build_clahe_h(ov2_ctx *ctx, ov2_pyr *p, const uint8_t *img_h, int stride, double clip_limit, int tiles_x, int tiles_y);
/* the same for `n_items` host images (one pointer each, rows `stride` apart) into items [0, n_items) of a batch pyramid: one repack into
 * pinned memory, ONE H2D, the batched kernels -- the right images of the keyframes a lock-step batch reaches together
 * (src/mapper.cpp:74-81 per keyframe).  clip_limit < 0: no CLAHE (use_clahe: 0).  Asynchronous like ov2_pyr_build_clahe_h.        */
int ov2_pyr_build_clahe_hb(ov2_ctx *ctx, ov2_pyr *p, int n_items, const uint8_t *const *img_h, int stride, double clip_limit, int tiles_x, int tiles_y);

/* ---- image rectification: CameraCalibration::rectifyImage ----------------------------------------
 * cv::remap(img, rect, undist_map_x_, undist_map_y_, cv::INTER_LINEAR) of src/camera_calibration.cpp:233-241, which
 * SlamManager::addNewMonoImage / addNewStereoImages run on every frame, left and right, before preprocessImage whenever
 * bdo_undist / bdo_stereo_rect is set (src/ov2slam.cpp:239-265).  CV_8UC1, INTER_LINEAR, BORDER_CONSTANT 0: OpenCV's own C++
 * path RESTATED (tests/remap_ref.py), not pinned against an OpenCV build; IPP's remap, which stock builds disable, is not the
 * canonical form.  The two map forms are the two the reference creates:
 *   OV2_MAP_F32    setUndistMap (:92 / :97), a CV_32FC1 pair: map1[y*w+x] = source x, map2[y*w+x] = source y (float).  Per
 *                  pixel sx = cvRound(x * 32.f), sy likewise (ties to even); ix = saturate_cast<short>(sx >> 5), a = sx & 31,
 *                  iy / b from sy (arithmetic shift, two's complement: negative coordinates floor).
 *   OV2_MAP_FIXED  setUndistStereoMap (:141 / :145), type 11: map1 = (ix, iy) int16 pairs (CV_16SC2), map2 = b * 32 + a as
 *                  uint16 (CV_16UC1).
 * With p00, p01, p10, p11 the source pixels at (ix, iy), (ix+1, iy), (ix, iy+1), (ix+1, iy+1), every tap outside the image 0:
 *   out = (p00*(32-a)*(32-b)*32 + p01*a*(32-b)*32 + p10*(32-a)*b*32 + p11*a*b*32 + (1 << 14)) >> 15
 * (OpenCV's BilinearTab_i; at (a, b) = (0, 0) its short table holds 32767 + a fix-up, which gives p00 for 8-bit pixels too).
 * ov2_rectmap_create checks the contract -- w, h in [2, 32767]; OV2_MAP_F32 values finite with |v| * 32 < 2^31; OV2_MAP_FIXED
 * map2 values < 1024: OV2_EINVAL otherwise -- and normalises either form, once, on the host, to one device representation
 * (6 B per pixel): there is one kernel path.  The handle is opaque and immutable; the caller's arrays are free on return.
 * A map must OUTLIVE every tracker it is set on (ov2_*_set_rectification) and every call it was passed to that is still in
 * flight: destroy it after them (or after ov2_*_set_rectification(t, NULL) / a synchronisation).  Computing the maps
 * (cv::initUndistortRectifyMap, cv::stereoRectify) happens once at start-up and stays with the caller.                     */
#define OV2_MAP_F32   0
#define OV2_MAP_FIXED 1
typedef struct ov2_rectmap ov2_rectmap;
int  ov2_rectmap_create(ov2_ctx *ctx, int w, int h, int form, const void *map1, const void *map2, ov2_rectmap **out);
void ov2_rectmap_destroy(ov2_rectmap *map);
/* rectifyImage on host buffers (rows src_stride / dst_stride bytes apart; only w bytes of a dst row are written): one H2D, the
 * kernel, one D2H, synchronising.  dst_h == src_h is allowed (the reference rectifies in place).                          */
int ov2_rectify_h(ov2_ctx *ctx, const ov2_rectmap *map, const uint8_t *src_h, int src_stride, uint8_t *dst_h, int dst_stride);
/* n_items device images `src_item_stride` bytes apart (rows src_pitch apart) -> dst likewise; the map entries are read once per
 * work-group and reused for its items.  Asynchronous on ctx's stream; src and dst must not overlap.  Whole-dword stores when
 * dst_d, dst_pitch and dst_item_stride are multiples of 4 (byte stores otherwise, same result).                           */
int ov2_rectify_d(ov2_ctx *ctx, const ov2_rectmap *map, const uint8_t *src_d, size_t src_pitch, size_t src_item_stride, int n_items,
                  uint8_t *dst_d, size_t dst_pitch, size_t dst_item_stride);
/* The right image(s) of a stereo keyframe (src/ov2slam.cpp:255-256, then src/mapper.cpp:74-81): n_items RAW host images (one
 * pointer each, rows `stride` apart) into items [0, n_items) of `p` -- ONE H2D, the remap, then what ov2_pyr_build_clahe_h /
 * _hb (use_clahe != 0) or ov2_pyr_build_h (use_clahe == 0: clip_limit / tiles ignored) do with the rectified frames.
 * Asynchronous like those; OV2_EINVAL when map and pyramid differ in size.                                                 */
int ov2_pyr_build_rect_h(ov2_ctx *ctx, ov2_pyr *p, const ov2_rectmap *map, int n_items, const uint8_t *const *img_h, int stride,
                         int use_clahe, double clip_limit, int tiles_x, int tiles_y);

/* ---- Lucas-Kanade --------------------------------------------------
 * ov2_lk_track replaces one cv::calcOpticalFlowPyrLK(prevPyr, nextPyr, prevPts,
 * nextPts, status, err, Size(win,win), max_level, TermCriteria(COUNT+EPS,
 * max_iter, eps), flags, 1e-4)  -- src/feature_tracker.cpp:66-69, :113-116.
 * flags: OV2_LK_USE_INITIAL_FLOW | OV2_LK_GET_MIN_EIGENVALS (the only
 * combination the reference uses); without GET_MIN_EIGENVALS err is left 0.
 * All point buffers are host memory, n points per batch item, batch items
 * contiguous (n_per_item[b] points for item b stored at offset b*n_max).
 */
#define OV2_LK_USE_INITIAL_FLOW   4
#define OV2_LK_GET_MIN_EIGENVALS  8

int ov2_lk_track(ov2_ctx *ctx, const ov2_pyr *prev, const ov2_pyr *next,
                 int win, int max_level, int max_iter, float eps, int flags,
                 const float *prev_xy_h, float *next_xy_inout_h, int n,
                 uint8_t *status_h, float *err_h, int *iters_h /* per point, may be NULL */);

/* ov2_fb_klt replaces FeatureTracker::fbKltTracking (src/feature_tracker.cpp:35-137):
 * forward LK (max_level = nbpyrlvl, clamped to the pyramid), status / err>err_th /
 * 1-px border filter, backward LK at level 0 from the tracked point with the
 * original keypoint as initial guess, reject if |kp - back| > fb_dist.
 * One fused kernel launch.  prior_xy_inout_h: in = initial guess, out = tracked
 * position (entries whose forward level-0 step was skipped keep OpenCV's
 * semantics).  n == 0 returns OV2_OK and touches nothing (:43-46).
 * stats (may be NULL): [0] = total GN iterations, [1] = (point,level) patch builds. */
int ov2_fb_klt(ov2_ctx *ctx, const ov2_pyr *prev, const ov2_pyr *cur,
               int win, int nbpyrlvl, int max_iter, float eps, float err_th, float fb_dist,
               const float *kps_xy_h, float *prior_xy_inout_h, int n,
               uint8_t *status_h, long long stats[2]);

/* Device-resident, batched form used by the offline batch-of-sequences path and
 * by bench.py: kps / priors / status live in HBM, item b uses points
 * [b*n_max, b*n_max + n_per_item_d[b])  (n_per_item_d == NULL -> n_max each).
 * stats_d (may be NULL): 2 x int64 accumulated with atomics (zero it yourself). */
int ov2_fb_klt_d(ov2_ctx *ctx, const ov2_pyr *prev, const ov2_pyr *cur,
                 int win, int nbpyrlvl, int max_iter, float eps, float err_th, float fb_dist,
                 const float *kps_xy_d, float *prior_xy_inout_d, int n_max, const int *n_per_item_d,
                 uint8_t *status_d, long long *stats_d);

/* ---- single-sequence tracker: preprocessImage + kltTracking ----------------------------------
 * One object per camera stream that owns what VisualFrontEnd keeps between frames -- prev_pyr_ / cur_pyr_
 * (src/visual_front_end.hpp) -- plus pinned staging buffers and, optionally, a captured hipGraph of the whole
 * per-frame enqueue.  It replaces, per frame, on the SLAM thread:
 *   VisualFrontEnd::preprocessImage  src/visual_front_end.cpp:1143-1177  (pyramid swap :1169, CLAHE :1159,
 *                                                                         cv::buildOpticalFlowPyramid :1172)
 *   VisualFrontEnd::kltTracking      src/visual_front_end.cpp:132-275    (both fbKltTracking calls :196 / :242, the
 *                                                                         retry of lost prior tracks :213-217 and the
 *                                                                         "motion model is wrong" rule :225-230)
 * with ONE H2D of the frame, ONE H2D of the keypoint block, five small kernels, ONE LK launch, ONE D2H and ONE
 * host synchronisation.  Results are identical to calling ov2_pyr_build_clahe_h + ov2_fb_klt twice.           */
typedef struct ov2_tracker ov2_tracker;
typedef struct {
    int w, h;                    /* image size                                                          */
    int win;                     /* nklt_win_size (9)                                                   */
    int nklt_pyr_lvl;            /* pyramid levels above 0 (3): full-pyramid pass                       */
    int prior_pyr_lvl;           /* nbpyrlvl of the 3-D-prior pass (1, visual_front_end.cpp:188)        */
    int max_iter; float eps;     /* klt_convg_crit_: nmax_iter (30), fmax_px_precision (0.01)           */
    float err_th, fb_dist;       /* nklt_err (30), fmax_fbklt_dist (0.5)                                */
    int use_clahe; double clahe_clip; int tiles_x, tiles_y;   /* use_clahe, fclahe_val, (w/50, h/50)    */
    int n_max;                   /* keypoints per fused launch (>= nbmaxkps; the adapters pass 2 x nbmaxkps).  NOT a
                                    limit on n: a frame can carry more than nbmaxkps keypoints (pruning happens at the
                                    next keyframe, src/map_manager.cpp:74); keypoints beyond n_max run through further
                                    launches of the same kernel, n_max at a time, with identical results              */
    int use_graph;               /* 1: replay a captured hipGraph per frame (falls back to plain enqueue
                                    when the context's stream cannot be captured)                       */
} ov2_tracker_config;

int  ov2_tracker_create(ov2_ctx *ctx, const ov2_tracker_config *cfg, ov2_tracker **out);
void ov2_tracker_destroy(ov2_tracker *t);
/* Pinned staging image the next frame may be written into directly (camera driver / decoder / cv::Mat header
 * over it): a frame passed from there skips the host-side copy.  *stride receives its pitch.               */
uint8_t *ov2_tracker_image_buffer(ov2_tracker *t, int *stride);
/* preprocessImage: swap prev/cur, H2D of the frame, CLAHE (if configured) + pyramid build.  ASYNCHRONOUS: returns
 * after the enqueue so the host can run its motion model while the GPU works; the image is staged through the
 * pinned buffer first, so img_h may be reused immediately.                                                 */
int  ov2_tracker_preprocess(ov2_tracker *t, const uint8_t *img_h, int stride);
/* kltTracking on (prev, cur) of the tracker.  has_prior_h[i] != 0: keypoint i carries a 3-D prior
 * (prior_xy_h[i] = projected map point) and is tracked on prior_pyr_lvl levels first; otherwise pass
 * prior_xy_h[i] = kps_xy_h[i] like the reference (:180-182).  klt_use_prior = 0 ignores has_prior_h.
 * out_xy_h[i]: tracked position (the value the reference hands to updateKeypoint, :204 / :256);
 * status_h[i]: bit 0 = tracked, bit 1 = lost on the prior pass and re-tracked on the full pyramid;
 * *p3p_req (may be NULL): 1 when fewer than a third of the prior tracks were good (bp3preq_, :225-230) -- the lost
 * prior tracks are then re-run from the keypoints themselves in a second launch, exactly like the reference.
 * Blocking (one synchronisation; one more per n_max keypoints beyond the first n_max).  n == 0 returns OV2_OK.     */
int  ov2_tracker_klt(ov2_tracker *t, const float *kps_xy_h, const float *prior_xy_h, const uint8_t *has_prior_h, int n,
                     int klt_use_prior, float *out_xy_h, uint8_t *status_h, int *p3p_req);
/* preprocess + klt in one enqueue (one graph launch when use_graph): the per-frame call of the drop-in.
 * The first frame after creation only builds the pyramid (nothing to track against): status_h is zeroed.   */
int  ov2_tracker_track_frame(ov2_tracker *t, const uint8_t *img_h, int stride, const float *kps_xy_h,
                             const float *prior_xy_h, const uint8_t *has_prior_h, int n, int klt_use_prior,
                             float *out_xy_h, uint8_t *status_h, int *p3p_req);
/* Optional: Frame::computeKeypoint (src/frame.cpp:246-254: undistortImagePoint + bearing vector, what the reference runs for
 * every keypoint it has just tracked, updateKeypoint) for every output position INSIDE the per-frame enqueue -- no second call,
 * no second synchronisation.  Same arguments as ov2_compute_keypoints.  Re-captures the tracker's graphs: call it right after
 * ov2_tracker_create.  ov2_tracker_last_keypoints then returns unpx (2 floats) / bv (3 doubles) per keypoint of the LAST
 * ov2_tracker_klt / _track_frame call (entries of untracked keypoints are computed from their last forward position).   */
int  ov2_tracker_set_calibration(ov2_tracker *t, int model, const double K[4], const double *D, int nD, const double iK[9]);
int  ov2_tracker_last_keypoints(const ov2_tracker *t, int n, float *unpx_xy_h, double *bv_xyz_h);
/* Optional: rectifyImage inside the per-frame enqueue.  From this call on the frames handed to ov2_tracker_preprocess /
 * _track_frame are RAW (distorted): each is uploaded to a buffer of its own (allocated by the first such call) and remapped, as
 * one more kernel of the same enqueue -- one more node of the captured graph, the chain stays linear -- before CLAHE / level 0.
 * The tracker's device frame then holds the RECTIFIED image: ov2_tracker_describe_brief and the detectors on the tracker's
 * pyramid see what the reference's imraw / im hold after rectifyImage.  map == NULL switches it off again (the frames are then
 * taken as they come, and every call enqueues exactly what it did before).  The map must match the tracker's w x h
 * (OV2_EINVAL) and outlive its use here.  Synchronises and re-captures the graphs like ov2_tracker_set_calibration.        */
int  ov2_tracker_set_rectification(ov2_tracker *t, const ov2_rectmap *map);
/* the tracker's pyramids (valid until the next preprocess), e.g. for createKeyframe / stereo matching / detection */
const ov2_pyr *ov2_tracker_cur_pyr(const ov2_tracker *t);
const ov2_pyr *ov2_tracker_prev_pyr(const ov2_tracker *t);
int  ov2_tracker_frames(const ov2_tracker *t);     /* frames preprocessed so far */
int  ov2_tracker_uses_graph(const ov2_tracker *t); /* 1 when the graph path is active */

/* ---- lock-step tracker: `batch` camera streams advance ONE FRAME PER CALL ---------------------------------
 * The offline / batch mode of the reference's benchmark protocol (benchmark_scripts/euroc_bench.sh:3-27 runs whole sequences one
 * after the other; BASELINE.json configs[4] shards them over GPUs): a rank that owns several sequences does not need their frames
 * one stream at a time.  One stream is a chain of ~10 small dependent launches per frame and a rank's streams together saturate
 * the launch rate with the CUs ~5 % busy (profiles/archive/r4_stream_concurrency.txt); here every launch of the per-frame enqueue --
 * frame upload, CLAHE, pyramid, the fused kltTracking kernel (both fbKltTracking calls + retry), Frame::computeKeypoint -- covers
 * all streams at once: same kernels as ov2_tracker_*, grid extended by the batch item, ONE synchronisation per step.
 * Results per item are bit-identical to an ov2_tracker fed the same frames / keypoints (tests/test_gpu_lockstep.py).
 *   items [0, n_active) take part in a call (sequences of different length: order them longest first and shrink n_active as
 *   they end); the state of the other items is not touched.
 *   point arrays hold cfg->n_max slots per item: item b's points are [b*n_max, b*n_max + n_h[b]); n_h[b] <= n_max.
 *   images: img_h[b] = frame of item b, rows `stride` bytes apart.  Three pinned staging sets exist (which = 0 / 1 / 2,
 *   ov2_btracker_image_buffer); frames passed from the slots of one set are not copied on the host.
 *   Look-ahead (optional; an offline host knows the next frames): the step is a three-stage pipeline on three streams --
 *     ov2_btracker_upload(which)    H2D of a filled staging set on the tracker's copy stream
 *     ov2_btracker_prepare(which)   preprocessImage (CLAHE + pyramid) of that set on the tracker's prep stream, into the pyramid set
 *                                   that becomes cur_pyr_ when the frame is tracked
 *     ov2_btracker_track_frame      with exactly those slots as img_h[]: only kltTracking + computeKeypoint remain (its stream waits
 *                                   for the pyramids); with other frames, or without the look-ahead calls, everything runs in order.
 *   A host loop: fill set (f+2)%3 [reader threads] -> upload((f+2)%3) -> prepare((f+1)%3) -> track_frame(frame f = set f%3).
 *   Results do not depend on which form is used.
 * hipGraph replay (cfg->use_graph) is not used here: n_active changes the grids.                                          */
typedef struct ov2_btracker ov2_btracker;
int  ov2_btracker_create(ov2_ctx *ctx, const ov2_tracker_config *cfg, int batch, ov2_btracker **out);
void ov2_btracker_destroy(ov2_btracker *t);
int  ov2_btracker_batch(const ov2_btracker *t);
int  ov2_btracker_frames(const ov2_btracker *t);
/* pinned slot of item `item` in staging set `which` (0 / 1 / 2); *stride receives its pitch */
uint8_t *ov2_btracker_image_buffer(ov2_btracker *t, int which, int item, int *stride);
/* asynchronous H2D of items [0, n_active) of staging set `which` (the caller has filled the slots); the next
 * ov2_btracker_prepare / ov2_btracker_track_frame of exactly those slots consumes the uploaded copy                   */
int  ov2_btracker_upload(ov2_btracker *t, int which, int n_active);
/* asynchronous preprocessImage of items [0, n_active) of staging set `which` for an ov2_btracker_track_frame to come: frames are
 * prepared in order, at most two may wait (the one about to be tracked and the one after it), and once a frame is prepared the
 * track_frame calls must consume exactly the prepared slots.  It overwrites the oldest pyramid set: see ov2_btracker_pyramid_sets   */
int  ov2_btracker_prepare(ov2_btracker *t, int which, int n_active);
/* Frame::computeKeypoint inside the per-step enqueue, as ov2_tracker_set_calibration (one calibration: the sequences of a batch
 * come from one camera rig)                                                                                            */
int  ov2_btracker_set_calibration(ov2_btracker *t, int model, const double K[4], const double *D, int nD, const double iK[9]);
/* rectifyImage inside the per-step enqueue, as ov2_tracker_set_rectification (one map: the sequences of a batch come from one
 * camera rig): the frames of ov2_btracker_track_frame / _upload / _prepare are RAW from this call on.  They are uploaded to a set
 * of three raw buffers (allocated by the first such call) and remapped for all active items in one launch before CLAHE / level 0 --
 * on the prep stream for ov2_btracker_prepare, on the context's stream otherwise; ov2_btracker_describe_brief then reads the
 * RECTIFIED frames.  map == NULL switches it off.  Call it between steps: it synchronises the tracker's streams, voids
 * uploads started ahead (they are repeated in order) and returns OV2_EINVAL while prepared frames wait or a step is open.   */
int  ov2_btracker_set_rectification(ov2_btracker *t, const ov2_rectmap *map);
/* preprocessImage + kltTracking of items [0, n_active): the lock-step form of ov2_tracker_track_frame, same per-item semantics
 * (first frame: pyramids only; has_prior_h / klt_use_prior / status bits / p3p_req[b] as there, the "motion model is wrong" retry
 * of visual_front_end.cpp:225-230 included).  Blocking: one synchronisation.                                             */
int  ov2_btracker_track_frame(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride, const float *kps_xy_h,
                              const float *prior_xy_h, const uint8_t *has_prior_h, const int *n_h, int klt_use_prior,
                              float *out_xy_h, uint8_t *status_h, int *p3p_req);
/* The same step in two halves: _begin enqueues it (frames, pre-processing or the wait for the prepared pyramids, the tracking
 * kernels) and returns; _end waits for it, returns the results and applies the p3p rule.  Between the two the host is free -- an
 * offline driver issues ov2_btracker_upload / ov2_btracker_prepare of the frames to come there, so that their enqueue cost runs beside
 * the tracking kernels instead of before them.  kps_xy_h / has_prior_h must stay valid until _end (the p3p rule re-reads them).
 * ov2_btracker_track_frame = _begin + _end.                                                                              */
int  ov2_btracker_track_frame_begin(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride, const float *kps_xy_h,
                                    const float *prior_xy_h, const uint8_t *has_prior_h, const int *n_h, int klt_use_prior);
int  ov2_btracker_track_frame_end(ov2_btracker *t, float *out_xy_h, uint8_t *status_h, int *p3p_req);
/* unpx (2 floats) / bv (3 doubles) of the first n keypoints of item `item` from the LAST ov2_btracker_track_frame */
int  ov2_btracker_last_keypoints(const ov2_btracker *t, int item, int n, float *unpx_xy_h, double *bv_xyz_h);
/* MapManager::extractKeypoints on the current frame of items [0, n_active) in one call (all sequences of a lock-step batch reach
 * their keyframes together): ov2_detect_singlescale_batch_d / ov2_detect_grid_fast_batch_d on level 0 of the current pyramids
 * with host buffers -- cur_xy_h: n_max slots per item, ncur_h[b] of them valid; out_xy_h: out_cap slots per item
 * (>= 2*(w/cell)*(h/cell), FAST: (w/cell)*(h/cell)); quality_inout / fast_th_inout: one adaptive state per item.          */
int  ov2_btracker_detect_singlescale(ov2_btracker *t, int n_active, int cell, const float *cur_xy_h, const int *ncur_h, const int roi[4],
                                     double *quality_inout, int do_subpix, float *out_xy_h, int out_cap, int *out_n_h);
int  ov2_btracker_detect_grid_fast(ov2_btracker *t, int n_active, int cell, const float *cur_xy_h, const int *ncur_h, int *fast_th_inout,
                                   int mask_mode, int do_subpix, float *out_xy_h, int out_cap, int *out_n_h);
/* the current / previous frame's pyramids: the whole batch, or item `item` as a batch-1 view (owned by the tracker; valid until that
 * pyramid set comes round again, see ov2_btracker_pyramid_sets) -- what the mapper context passes to ov2_stereo_match as `left` */
/* How many pyramid sets the tracker rotates through (8): the pyramids of frame f are overwritten by the pre-processing of frame
 * f + sets -- ov2_btracker_track_frame of that frame, or the ov2_btracker_prepare call for it.  A consumer on another context (the
 * mapper's stereo matching of keyframe f) must be done before the caller issues that call. */
int  ov2_btracker_pyramid_sets(const ov2_btracker *t);
const ov2_pyr *ov2_btracker_cur_pyr(const ov2_btracker *t);
const ov2_pyr *ov2_btracker_prev_pyr(const ov2_btracker *t);
const ov2_pyr *ov2_btracker_cur_item(const ov2_btracker *t, int item);
const ov2_pyr *ov2_btracker_prev_item(const ov2_btracker *t, int item);

/* ---- keypoint detection ---------------------------------------------
 * mask_mode for the FAST grid detector: the reference passes a
 * CV_32F mask to cv::FastFeatureDetector::detect, which reads it as bytes.     */
#define OV2_MASK_AS_EXECUTED 0
#define OV2_MASK_INTENDED    1

/* FeatureExtractor::detectGridFAST (src/feature_extractor.cpp:443-570).
 * fast_th_inout mirrors the member nfast_th_ (adapted at :546-552).
 * out_xy_h capacity (w/cell)*(h/cell) points.  do_subpix=0 skips cv::cornerSubPix. */
int ov2_detect_grid_fast(ov2_ctx *ctx, const uint8_t *img_h, int w, int h, int stride, int cell,
                         const float *cur_xy_h, int ncur, int *fast_th_inout, int mask_mode,
                         int do_subpix, float *out_xy_h, int *out_n);

/* FeatureExtractor::detectSingleScale (src/feature_extractor.cpp:288-440).
 * roi = {x, y, width, height} (the 5-px border rect of camera_calibration.cpp:72-73).
 * quality_inout mirrors dmaxquality_ (:418-423).  out_xy_h capacity 2*(w/cell)*(h/cell). */
int ov2_detect_singlescale(ov2_ctx *ctx, const uint8_t *img_h, int w, int h, int stride, int cell,
                           const float *cur_xy_h, int ncur, const int roi[4], double *quality_inout,
                           int do_subpix, float *out_xy_h, int *out_n);

/* Device-resident forms of the two detectors: the image is level 0 of batch item `item` of a pyramid that already lives in
 * HBM.  At a keyframe the reference passes cur_img_ -- the CLAHE'd frame preprocessImage also built cur_pyr_ from -- to
 * MapManager::extractKeypoints (src/map_manager.cpp:286-341, detector choice :312-320): that image IS level 0 of the
 * tracker's current pyramid (ov2_tracker_cur_pyr), so a keyframe costs no upload.  Results are identical to the host-image
 * forms on the same pixels.  One host synchronisation per call.                                                          */
int ov2_detect_grid_fast_d(ov2_ctx *ctx, const ov2_pyr *pyr, int item, int cell, const float *cur_xy_h, int ncur,
                           int *fast_th_inout, int mask_mode, int do_subpix, float *out_xy_h, int *out_n);
int ov2_detect_singlescale_d(ov2_ctx *ctx, const ov2_pyr *pyr, int item, int cell, const float *cur_xy_h, int ncur,
                             const int roi[4], double *quality_inout, int do_subpix, float *out_xy_h, int *out_n);

/* The same detectors on EVERY batch item of the pyramid in one call (the offline batch-of-sequences mode: all sequences reach
 * a keyframe together).  Everything but the adaptive per-sequence state stays on the device:
 *   cur_xy_d   device, batch x cur_cap points (x, y): the items' current keypoints; ncur_d device, batch counts (NULL: none)
 *   out_xy_d   device, batch x out_cap points; out_cap >= (w/cell)*(h/cell) for FAST, twice that for single scale
 *   quality_inout / fast_th_inout   host, one entry per item (dmaxquality_ / nfast_th_ of that sequence), updated like the
 *              single-image forms; out_n_h host, points written per item.
 * Results per item are identical to the single-image forms.  One host synchronisation per call.                        */
int ov2_detect_singlescale_batch_d(ov2_ctx *ctx, const ov2_pyr *pyr, int cell, const float *cur_xy_d, int cur_cap, const int *ncur_d,
                                   const int roi[4], double *quality_inout, int do_subpix, float *out_xy_d, int out_cap, int *out_n_h);
int ov2_detect_grid_fast_batch_d(ov2_ctx *ctx, const ov2_pyr *pyr, int cell, const float *cur_xy_d, int cur_cap, const int *ncur_d,
                                 int *fast_th_inout, int mask_mode, int do_subpix, float *out_xy_d, int out_cap, int *out_n_h);

/* cv::cornerSubPix(im, pts, Size(hw,hw), Size(-1,-1), TermCriteria(EPS+MAX_ITER, max_iter, eps))
 * src/feature_extractor.cpp:434, :564 (hw = 3, 30, 0.01).  In place.             */
int ov2_corner_subpix(ov2_ctx *ctx, const uint8_t *img_h, int w, int h, int stride,
                      float *xy_inout_h, int n, int half_win, int max_iter, double eps);

/* ---- GFTT (Shi-Tomasi) detection --------------------------------------
 * FeatureExtractor::detectGFTT (src/feature_extractor.cpp:104-221, the use_shi_tomasi branch of MapManager::extractKeypoints,
 * src/map_manager.cpp:312-314) with its setMask helper (:575-584).  The four members it reads are passed explicitly:
 * ov2_gftt_params_init derives nmindist = nmaxdist / 2 (truncated) and dminquality = dmaxquality / 2 like the constructor (:79-83).
 *   1. ncur >= nmaxpts: no points.  nb2detect = nbmax != -1 ? nbmax : nmaxpts - ncur.
 *   2. pass 1: mask = roi (all pixels when NULL), zeroed by a filled cv::circle of radius nmaxdist at cvRound of every current
 *      keypoint; goodFeaturesToTrack(maxCorners nb2detect, quality dminquality, minDistance nmaxdist, blockSize 3, gradSize 3):
 *        eig  = cornerMinEigenVal(im, 3, 3) over the whole image, REFLECT_101 (no blur; Sobel dy order: OV2_OPT_SOBEL_DY_ORDER)
 *        thr  = (float)(maxVal * quality), maxVal the maximum of eig where the mask is non-zero (0 when there is no such pixel)
 *        candidates: interior pixels (1 <= x <= w-2, 1 <= y <= h-2) with t != 0, t == 3x3 max of t and mask != 0, where
 *              t = eig > thr ? eig : 0
 *        order: value descending; EQUAL values: the later pixel (higher y*w + x) first -- OpenCV 4.x greaterThanPtr.  OpenCV 3.x
 *              compares values only under an unstable std::sort; that order is not reproduced.
 *        greedy: a candidate is dropped when an accepted point lies at dx^2 + dy^2 < minDistance^2; stop at maxCorners.
 *      then cornerSubPix(3x3, 30 iterations, eps 0.01) when do_subpix.
 *   3. n1 >= 0.66 * nb2detect or nb2detect < 20: done.  Otherwise pass 2 with mask = roi minus discs of radius nmindist at the
 *      current keypoints AND the (refined) pass-1 points, quality dmaxquality, minDistance nmindist, maxCorners nb2detect - n1;
 *      its points follow the pass-1 points.
 * The eig map is shared by both passes.  The arithmetic is restated from the public OpenCV source and NOT pinned against an OpenCV
 * binary (the status of detectSingleScale's response); IPP / SIMD builds of OpenCV may round differently.
 * Arguments: nbmax -1 or >= 1 (0, which OpenCV reads as "no limit", and < -1 -> OV2_EINVAL; the reference never passes them);
 * out_cap >= nb2detect (OV2_EINVAL), nb2detect <= 4096 and nmaxdist <= 63 (OV2_EUNSUPPORTED); images at least 16 x 16
 * (OV2_EUNSUPPORTED); an empty image (NULL, w or h <= 0) gives 0 points.  One host synchronisation per call.
 * Scratch: the context's grow-only device buffer, 21 B per pixel and item + the output lists (7.6 MB for 752 x 480); batches run in
 * chunks of at most 256 MB of it (at least one item).                                                                         */
typedef struct { int nmaxpts, nmaxdist, nmindist; double dminquality, dmaxquality; } ov2_gftt_params;
int ov2_gftt_params_init(int nmaxpts, int nmaxdist, double dmaxquality, ov2_gftt_params *out);
/* host image; roi_h: NULL or a w x h byte mask (rows roi_stride bytes apart, non-zero = allowed); cur_xy_h: ncur points */
int ov2_detect_gftt(ov2_ctx *ctx, const uint8_t *img_h, int w, int h, int stride, const uint8_t *roi_h, int roi_stride,
                    const ov2_gftt_params *params, const float *cur_xy_h, int ncur, int nbmax, int do_subpix,
                    float *out_xy_h, int out_cap, int *out_n);
/* level 0 of batch item `item` of a device pyramid (the tracker's current CLAHE'd frame): no image upload */
int ov2_detect_gftt_d(ov2_ctx *ctx, const ov2_pyr *pyr, int item, const uint8_t *roi_h, int roi_stride,
                      const ov2_gftt_params *params, const float *cur_xy_h, int ncur, int nbmax, int do_subpix,
                      float *out_xy_h, int out_cap, int *out_n);
/* every item of the pyramid: roi_d device mask shared by all items (NULL: none); cur_xy_d cur_cap points per item, ncur_d[b] valid
 * (NULL: none); nbmax_h host, one per item; out_xy_d out_cap points per item, out_cap >= max over items of (nbmax, or nmaxpts
 * where nbmax is -1); out_n_h host counts.  Identical per item to the single-image forms.                                       */
int ov2_detect_gftt_batch_d(ov2_ctx *ctx, const ov2_pyr *pyr, const uint8_t *roi_d, int roi_stride, const ov2_gftt_params *params,
                            const float *cur_xy_d, int cur_cap, const int *ncur_d, const int *nbmax_h, int do_subpix,
                            float *out_xy_d, int out_cap, int *out_n_h);
/* lock-step form on the current frames of items [0, n_active) with host buffers (layout of ov2_btracker_detect_singlescale:
 * cur_xy_h n_max slots per item, out_xy_h out_cap slots per item); roi_h as in ov2_detect_gftt, shared by all items */
int ov2_btracker_detect_gftt(ov2_btracker *t, int n_active, const uint8_t *roi_h, int roi_stride, const ov2_gftt_params *params,
                             const float *cur_xy_h, const int *ncur_h, const int *nbmax_h, int do_subpix,
                             float *out_xy_h, int out_cap, int *out_n_h);
/* FeatureExtractor::setMask on a host mask: a filled cv::circle of radius dist (value 0) at cvRound(x), cvRound(y) of each point
 * (the pixels the kernels paint) */
int ov2_set_mask(uint8_t *mask, int w, int h, int stride, const float *xy, int n, int dist);

/* ---- BRIEF descriptors ----------------------------------------------
 * FeatureExtractor::describeBRIEF (src/feature_extractor.cpp:224-285): cv::xfeatures2d::BriefDescriptorExtractor with its defaults
 * (32 bytes, use_orientation = false), called twice per keyframe from MapManager::extractKeypoints on the RAW left image.  Per point:
 *   valid     28 <= rint(x) < w-28 and 28 <= rint(y) < h-28 (rint: half to even; NaN / inf never; w or h <= 56: none) -- the
 *             reference's empty cv::Mat for a rejected point (:263-278) is valid = 0; its descriptor is 32 zero bytes
 *   centre    cx = (int)(x + 0.5), cy = (int)(y + 0.5)
 *   bit t     S(ay, ax) < S(by, bx) for test pair t = {ay, ax, by, bx} (row offset first), S(dy, dx) = sum of the 9x9 pixels centred
 *             at (cy+dy, cx+dx); byte j = tests 8j..8j+7, the first one in the most significant bit
 * Exact integer arithmetic: results are bit-identical whatever the call form.  Restated from the public OpenCV source (brief.cpp,
 * keypoint.cpp), not yet confirmed against an OpenCV build (tools/ref_capture/capture_brief.cpp captures the comparison).  One case
 * is defined differently on purpose: odd w, x == w-28.5 exactly and a +24 column offset (rows alike) make OpenCV read past its
 * integral image; here a box only ever sums the pixels inside the image.
 * THE PATTERN IS CONTEXT STATE.  The built-in table (ov2slam_amd/csrc/brief_pattern.hpp, tools/gen_brief_pattern.py) is NOT OpenCV's:
 * the map only compares descriptors with each other, so any fixed table works there, but a host that mixes these descriptors with
 * OpenCV-computed ones (the reference's loop closer) must load OpenCV's table first (tests/golden/brief_pattern_opencv.npy, recovered
 * by tools/brief_pattern_from_probes.py).
 * Every describe call synchronises the host once.  Scratch: the context's grow-only buffers -- device: the image (host form, rows
 * padded to 256 B) + 41 B per point slot + 256 B per item; pinned host: 41 B per point slot.  n == 0 returns OV2_OK.            */
#define OV2_BRIEF_BYTES 32
/* pairs: 256 x {ay, ax, by, bx}; NULL restores the built-in table; an offset outside [-24, 24] -> OV2_EINVAL, previous table kept */
int ov2_brief_set_pattern(ov2_ctx *ctx, const int8_t *pairs);
int ov2_brief_get_pattern(ov2_ctx *ctx, int8_t *pairs);
/* host image (w x h, rows `stride` bytes apart), n points (x, y) -> desc_h n x 32 bytes, valid_h n flags (0 / 1) */
int ov2_describe_brief(ov2_ctx *ctx, const uint8_t *img_h, int w, int h, int stride, const float *xy_h, int n,
                       uint8_t *desc_h, uint8_t *valid_h);
/* n_items device images `item_stride` bytes apart (rows `pitch` bytes apart); device points, cap slots per item, n_d[b] of them valid
 * (n_d NULL: all cap; counts above cap are taken as cap); device outputs in the same slot layout (desc: 32 B per slot; slots past
 * n_d[b] are not written).  n_items <= 65535.                                                                                     */
int ov2_describe_brief_batch_d(ov2_ctx *ctx, const uint8_t *img_d, int w, int h, int pitch, size_t item_stride, int n_items,
                               const float *xy_d, int cap, const int *n_d, uint8_t *desc_d, uint8_t *valid_d);
/* the RAW frame of the tracker's current frame (the image given to the last preprocess / track_frame, before CLAHE -- already in HBM:
 * no upload; after ov2_tracker_set_rectification: that image rectified); valid until the next preprocess.  Needs one preprocessed frame. */
int ov2_tracker_describe_brief(ov2_tracker *t, const float *xy_h, int n, uint8_t *desc_h, uint8_t *valid_h);
/* the raw frames of the current lock-step step (the last ov2_btracker_track_frame), items [0, n_active) with n_active <= that step's;
 * host points / outputs with cap slots per item (n_h[b] valid; slots past n_h[b] untouched).  OV2_EINVAL once the staging set that
 * held those frames has been uploaded or prepared again (ov2_btracker_upload / _prepare of that set, or the next step): in the
 * look-ahead loop, describe right after the step.                                                                                 */
int ov2_btracker_describe_brief(ov2_btracker *t, int n_active, const float *xy_h, const int *n_h, int cap,
                                uint8_t *desc_h, uint8_t *valid_h);

/* ---- local bundle adjustment ----------------------------------------
 * Replaces the two ceres::Solve calls of Optimizer::localBA
 * (src/optimizer.cpp:479 and :618) on the anchored-inverse-depth problem built at
 * :128-407.  The adapter walks the map on the CPU (as the reference does) into
 * the flat arrays below.  Residual types follow src/ceres_parametrization.cpp.
 */
enum {
    OV2_RES_LEFT       = 0, /* DirectLeftSE3::ReprojectionErrorKSE3AnchInvDepth         :361-473 */
    OV2_RES_RIGHT      = 1, /* DirectLeftSE3::ReprojectionErrorRightCamKSE3AnchInvDepth :579-712 */
    OV2_RES_RIGHT_ANCH = 2, /* DirectLeftSE3::ReprojectionErrorRightAnchCamKSE3AnchInvDepth :476-577 */
    OV2_RES_PNP        = 3  /* DirectLeftSE3::ReprojectionErrorSE3 (fixed world point) :301-358 -- the factor of
                               MultiViewGeometry::ceresPnP, src/multi_view_geometry.cpp:492-586; uses res_kf, res_xyz,
                               res_uv, res_sigma and calib_l; res_lm is ignored */
};

typedef struct {
    int n_kf;                    /* keyframe poses Twc, [tx ty tz qx qy qz qw] each (se3_param_block.hpp:40-46) */
    const double *poses;         /* 7*n_kf                                        */
    const uint8_t *kf_const;     /* n_kf; 1 = SetParameterBlockConstant (optimizer.cpp:176-185, :229-246, :397-407) */
    int n_lm;                    /* anchored inverse-depth landmarks              */
    const double *invdepth;      /* n_lm                                          */
    const int *lm_anchor_kf;     /* n_lm; index into poses                        */
    const double *lm_anchor_uv;  /* 2*n_lm; undistorted anchor pixel              */
    int n_res;                   /* 2-row residual blocks                         */
    const uint8_t *res_type;     /* n_res; OV2_RES_*                              */
    const int *res_kf;           /* n_res; observing keyframe (unused for RIGHT_ANCH) */
    const int *res_lm;           /* n_res                                         */
    const double *res_uv;        /* 2*n_res; observed pixel                       */
    const double *res_sigma;     /* n_res; 2^scale (always 1 in the reference)    */
    const uint8_t *res_active;   /* n_res or NULL; 0 = residual block removed (optimizer.cpp:500-592) */
    const double *res_xyz;       /* 3*n_res; world point of OV2_RES_PNP blocks (ignored for the others); NULL if none */
    double calib_l[4];           /* fx fy cx cy, constant block                   */
    double calib_r[4];
    double T_rl[7];              /* right <- left extrinsic, [t q], constant block */
} ov2_ba_problem;

typedef struct {
    int max_iter;                /* 5 (robust pass) / 10 (L2 pass), optimizer.cpp:461, :611 */
    double function_tolerance;   /* 1e-3, :462                                    */
    double gradient_tolerance;   /* Ceres default 1e-10                           */
    double parameter_tolerance;  /* Ceres default 1e-8                            */
    double huber_delta;          /* sqrt(5.9915), :49; <= 0: no loss function     */
    double initial_radius;       /* 1e4  (Ceres initial_trust_region_radius)      */
    double max_radius;           /* 1e16                                          */
    double min_radius;           /* 1e-32                                         */
    double min_lm_diagonal;      /* 1e-6                                          */
    double max_lm_diagonal;      /* 1e32                                          */
    double min_relative_decrease;/* 1e-3                                          */
    int jacobi_scaling;          /* 1                                             */
    int max_consecutive_invalid_steps; /* 5                                       */
    double max_solver_time_s;    /* Ceres max_solver_time_in_seconds: 0.2 / 0.1 s in localBA when force_realtime (optimizer.cpp:464-468,
                                    :612), 5 ms in ceresPnP (multi_view_geometry.cpp:546), 10-20 ms in structureOnlyBA; <= 0 = no limit
                                    (the default: results are then independent of machine load).  The limit is checked by the host
                                    between chunks of 2 LM iterations; when it fires no further iteration is started and the solve
                                    returns the last accepted state with OV2_TERM_NO_CONVERGENCE, like Ceres' "maximum solver time" exit */
} ov2_ba_options;

enum {
    OV2_TERM_NO_CONVERGENCE = 0, OV2_TERM_FUNCTION_TOL = 1, OV2_TERM_PARAMETER_TOL = 2,
    OV2_TERM_GRADIENT_TOL = 3, OV2_TERM_MIN_RADIUS = 4, OV2_TERM_INVALID_STEPS = 5,
    OV2_TERM_FAILURE = 6
};

typedef struct {
    double *poses_out;           /* 7*n_kf                                        */
    double *invdepth_out;        /* n_lm                                          */
    double *chi2_last_eval;      /* n_res: chi2err_ cached by the last Evaluate */
    uint8_t *depthpos_last_eval; /* n_res: isdepthpositive_ likewise              */
    int iterations;              /* LM iterations executed (Ceres summary.iterations.size()-1) */
    int num_successful_steps;
    double initial_cost, final_cost;
    int termination;             /* OV2_TERM_*                                    */
    double solve_ms;             /* device time of the solve (HIP events)         */
} ov2_ba_result;

void ov2_ba_default_options(ov2_ba_options *o);
/* One ceres::Solve: H2D of the problem, the whole LM loop on the device (a fixed kernel sequence,
 * one host synchronisation), D2H of the result.  When p->res_active is given, the entries of
 * r->chi2_last_eval / r->depthpos_last_eval that belong to inactive residual blocks are IN/OUT:
 * they keep the caller's values, like the cached chi2err_ of a removed residual block (N4).
 * Size: up to ~90 optimised keyframes the reduced system is solved in one work-group's LDS; beyond that (a loop-closure
 * fullBA) a sparse-W / HBM-Cholesky path takes over by itself, same results, up to 1024 optimised keyframes (the dense reduced
 * system: 3 x 302 MB at the cap), with or without OV2_RES_PNP blocks; past that OV2_EUNSUPPORTED with a message, nothing enqueued. */
int  ov2_ba_solve(ov2_ctx *ctx, const ov2_ba_problem *p, const ov2_ba_options *o, ov2_ba_result *r);

/* Iteration trace of the LAST one-problem solve of this context (OV2_OPT_BA_TRACE = 1): one entry per iteration that Ceres'
 * TrustRegionMinimizer pushes into Solver::Summary::iterations (Thirdparty/ceres-solver/internal/ceres/trust_region_minimizer.cc:313-337;
 * include/ceres/iteration_callback.h:45-150) -- entry 0 is the starting point; an iteration that ends the solve inside the loop
 * (parameter / function tolerance, :706-748) is not recorded, as in Ceres.  gradient_norm is NaN (the device forms the max norm only).
 * *n = entries recorded by the solve (the library keeps the first 64), buf receives min(*n, 64, cap).  tests/test_gpu_ba.py compares it
 * with the oracle's trace; tests/test_reference_trlm.py compares both with Ceres' own loop compiled in place.                       */
typedef struct {
    int iteration, step_is_valid, step_is_successful, reserved_;
    double cost, cost_change, gradient_max_norm, gradient_norm, step_norm, relative_decrease, trust_region_radius;
} ov2_ba_iter;
int  ov2_ba_get_trace(ov2_ctx *ctx, ov2_ba_iter *buf, int cap, int *n);

/* Same solve on a problem that is already resident in HBM (upload once, solve many times from the
 * same initial parameters); used by bench.py so that the timed region starts with inputs in HBM. */
typedef struct ov2_ba_dev ov2_ba_dev;
int  ov2_ba_create(ov2_ctx *ctx, const ov2_ba_problem *p, ov2_ba_dev **out);
int  ov2_ba_solve_resident(ov2_ctx *ctx, ov2_ba_dev *dev, const ov2_ba_options *o, ov2_ba_result *r);
void ov2_ba_destroy(ov2_ba_dev *dev);

/* Optimizer::localBA's whole solve stage (src/optimizer.cpp:436-735) in ONE call with the problem resident in HBM between the
 * two ceres::Solve calls: one sort + upload of the residual blocks, pass 1 (Huber unless !use_robust_cost), the outlier test
 * on the values cached by the last Evaluate (chi2err_ > robust_mono_th or depth <= 0, :492-594) and the removal
 * of the outlier blocks ON THE DEVICE, pass 2 (only if apply_l2_after_robust && use_robust_cost && !stop_requested && outliers
 * were found, :603-604; loss reset to L2 only when a left AND a right-camera block remain, :606-608 -- mono runs keep Huber),
 * the second outlier test on the blocks still in the problem (:637-735), one download.  Two ov2_ba_solve calls return the same
 * (tests/test_gpu_ba.py) but sort, upload and download the residual blocks twice: 11.5 -> see bench `localba_two_pass_stereo`.
 * pass1 / pass2 carry the iteration caps and tolerances (their huber_delta is ignored: the protocol sets it).  Inverse-depth
 * problems without OV2_RES_PNP blocks; same size limits as ov2_ba_solve.                                                */
typedef struct {
    double robust_mono_th;       /* 5.9915 (slam_params.hpp robust_mono_th_)                              */
    int use_robust_cost;         /* localBA's buse_robust_cost argument                                   */
    int apply_l2_after_robust;   /* apply_l2_after_robust_                                                */
    int stop_requested;          /* a stop that is already known at entry (ORed with *stop_flag)          */
    const volatile int *stop_flag;/* or NULL.  The LIVE Optimizer::bstop_localba_ (include/optimizer.hpp:48-49): the reference tests
                                    !stopLocalBA() AFTER its first ceres::Solve (:603-604) and Estimator::addNewKf raises the flag from
                                    another thread while pass 1 runs, so the library reads *stop_flag once, right before it decides
                                    on pass 2 (after pass 1 and the first outlier test), never at entry                              */
    ov2_ba_options pass1, pass2; /* max_iter 5 / 10, function_tolerance 1e-3 (:461-462, :611).  max_solver_time_s: the reference runs
                                    pass 1 with 0.2 s (0.4 s unless force_realtime, :463-467) and pass 2 with HALF of that (:612); the
                                    defaults here are 0 = no limit (results independent of machine load): an adapter that wants the
                                    reference's limits sets pass1.max_solver_time_s = t and pass2.max_solver_time_s = t / 2           */
} ov2_local_ba_options;
typedef struct {
    double *poses_out;           /* 7*n_kf                                                                */
    double *invdepth_out;        /* n_lm                                                                  */
    uint8_t *bad_obs;            /* n_res: 1 = outlier after the whole protocol (remove the observation)  */
    uint8_t *bad_after_pass1;    /* n_res or NULL: verdicts of the first test only                        */
    double *chi2_last_eval;      /* n_res or NULL (not downloaded)                                        */
    uint8_t *depthpos_last_eval; /* n_res or NULL                                                         */
    int l2_done;                 /* pass 2 ran (and succeeded)                                            */
    int pass2_error;             /* OV2_OK, or why pass 2 could not run: the call then still returns OV2_OK with the valid result of
                                    pass 1 + first outlier test in every output (what the reference keeps when its second Solve
                                    gives up); the message is in ov2_last_error()                                                    */
    int n_bad_pass1, n_bad_total;
    int iterations[2], num_successful_steps[2], termination[2];
    double initial_cost[2], final_cost[2];
    double solve_ms[2];          /* device time of each pass                                              */
    int status;                  /* OV2_OK, or this problem's error code (ABI 600).  ov2_local_ba: the value it returns.  ov2_local_ba_batch:
                                    every problem is attempted; r[i].status tells which results are valid and the call returns the
                                    first non-OK status in problem order (OV2_OK when all are).  The buffers of a problem whose
                                    input was rejected are not written                                                               */
} ov2_local_ba_result;
void ov2_local_ba_default_options(ov2_local_ba_options *o);
int  ov2_local_ba(ov2_ctx *ctx, const ov2_ba_problem *p, const ov2_local_ba_options *o, ov2_local_ba_result *r);
/* The same protocol for n problems at once -- the estimator side of the lock-step batch of sequences (BASELINE configs[4]; the
 * reference runs one Optimizer::localBA per sequence on that sequence's estimator thread, src/estimator.cpp:71-93).  Every kernel
 * of the solver is launched ONCE for the batch (grid.z = problem; a problem that has converged, or takes no second pass, drops
 * out inside the kernels), so n solves cost the launches of one and the one-work-group kernels (factorisation, trust-region
 * bookkeeping) run side by side.  p, o, r: n entries each; the entries of o share robust_mono_th, use_robust_cost,
 * apply_l2_after_robust, pass1 and pass2 (OV2_EINVAL otherwise) -- stop_requested / stop_flag are per problem and read after the
 * first pass of the batch.  Per problem the result is what ov2_local_ba returns for it (same device code; floating-point sums
 * over work-groups are grouped by the batch's grid: parity 1e-7, tests/test_gpu_ba_batch.py); solve_ms is the device time of
 * the batch's pass.  Problems the shared launches do not cover (more optimised keyframes than the LDS-resident path holds,
 * OV2_RES_PNP blocks, no landmarks, OV2_OPT_BA_DETERMINISTIC) are solved one after the other through ov2_local_ba in the same
 * call; *n_batched (or NULL) = how many shared the launches; a failure of one of them (r[i].status) does not stop the others.
 * Options that disagree (or robust_mono_th <= 0) are an error of the batch: every status is OV2_EINVAL and nothing runs.  A problem
 * whose input is rejected gets its own code and leaves the shared launches to the others; a failure of the shared launches
 * themselves (memory, a HIP error) is the status of every problem that shared them, and the problems solved alone still run.
 * max_solver_time_s is ONE host-clock budget for the batch's shared pass (the batch advances iteration by iteration, so a slow
 * window ends the pass for all): a caller that wants the reference's per-problem limit leaves it at 0 here, or calls ov2_local_ba
 * per problem.                                                                                                                 */
int  ov2_local_ba_batch(ov2_ctx *ctx, int n, const ov2_ba_problem *p, const ov2_local_ba_options *o, ov2_local_ba_result *r, int *n_batched);

/* ------------------------------------------------------------------ */
/* Optimizer::structureOnlyBA                                           */
/* ------------------------------------------------------------------ */
/* One ceres::Solve of Optimizer::structureOnlyBA (src/optimizer.cpp:2594-2781, called at
 * src/loop_closer.cpp:353 on the map points merged by a loop closure): 3-D world points
 * (PointXYZParametersBlock) are the only variables; every keyframe pose, both calibrations and the stereo
 * extrinsic are constant blocks.  Residual blocks:
 *   OV2_XYZ_LEFT   DirectLeftSE3::ReprojectionErrorKSE3XYZ          (left camera,  :2692-2702, :2719-2727)
 *   OV2_XYZ_RIGHT  DirectLeftSE3::ReprojectionErrorRightCamKSE3XYZ  (right camera through T_rl, :2704-2715)
 * Options: the reference uses DENSE_SCHUR / LM, max_num_iterations 10, function_tolerance 1e-3, Huber
 * sqrt(robust_mono_th) (:2599-2601, :2742-2758) -- fill an ov2_ba_options accordingly; its 10-20 ms
 * max_solver_time_in_seconds has no counterpart.  The function never changes poses.                    */
enum { OV2_XYZ_LEFT = 0, OV2_XYZ_RIGHT = 1 };
typedef struct {
    int n_kf;
    const double *poses;         /* 7*n_kf  [tx ty tz qx qy qz qw] of Twc (constant)          */
    int n_pts;
    const double *xyz;           /* 3*n_pts world points, initial values                      */
    int n_res;
    const uint8_t *res_type;     /* n_res   OV2_XYZ_*                                         */
    const int *res_kf;           /* n_res   observing keyframe                                */
    const int *res_pt;           /* n_res   observed point                                    */
    const double *res_uv;        /* 2*n_res undistorted pixel (unpx_ / runpx_)                */
    const double *res_sigma;     /* n_res   2^scale                                           */
    const uint8_t *res_active;   /* n_res or NULL                                             */
    double calib_l[4], calib_r[4], T_rl[7];
} ov2_sba_problem;
typedef struct {
    double *xyz_out;             /* 3*n_pts                                                   */
    double *chi2_last_eval;      /* n_res, in/out like ov2_ba_result (may be NULL)            */
    uint8_t *depthpos_last_eval; /* n_res, in/out (may be NULL)                               */
    int iterations, num_successful_steps;
    double initial_cost, final_cost;
    int termination;             /* OV2_TERM_*                                                */
    double solve_ms;
} ov2_sba_result;
int ov2_structure_ba(ov2_ctx *ctx, const ov2_sba_problem *p, const ov2_ba_options *o, ov2_sba_result *r);

/* ------------------------------------------------------------------ */
/* Bundle adjustment over 3-D points with variable poses (buse_inv_depth: 0) */
/* ------------------------------------------------------------------ */
/* One ceres::Solve of Optimizer::localBA / looseBA / fullBA when `buse_inv_depth: 0`: map points enter as
 * PointXYZParametersBlock (3 doubles, elimination group 0, src/optimizer.cpp:207-209) and every observation is a
 *   OV2_XYZ_LEFT   DirectLeftSE3::ReprojectionErrorKSE3XYZ          {calib, pose, X}            (:333-384, :366-375)
 *   OV2_XYZ_RIGHT  DirectLeftSE3::ReprojectionErrorRightCamKSE3XYZ  {calib_r, pose, T_rl, X}    (:347-357)
 * residual block with a VARIABLE keyframe pose (factors src/ceres_parametrization.cpp:107-298); kf_const marks the
 * SetParameterBlockConstant keyframes (:397-407).  Same options, termination codes and N4 outputs as ov2_ba_solve; the
 * Schur complement eliminates 3x3 point blocks.  No shipped parameter file selects this branch; the inverse-depth form
 * (ov2_ba_solve) is what every preset runs.  Limit: ~450 optimised keyframes (OV2_EUNSUPPORTED beyond): W stays dense in
 * this form (3 rows per wavefront in LDS); beyond ~90 keyframes its reduced system is factored by the same multi-kernel
 * Cholesky on HBM as ov2_ba_solve's large-problem path (which reaches 1024 keyframes with a sparse W).              */
typedef struct {
    int n_kf;
    const double *poses;         /* 7*n_kf  [tx ty tz qx qy qz qw] of Twc, initial values      */
    const uint8_t *kf_const;     /* n_kf; 1 = constant block (NULL: every pose variable)       */
    int n_pts;
    const double *xyz;           /* 3*n_pts world points, initial values                       */
    int n_res;
    const uint8_t *res_type;     /* n_res   OV2_XYZ_*                                          */
    const int *res_kf;           /* n_res   observing keyframe                                 */
    const int *res_pt;           /* n_res   observed point                                     */
    const double *res_uv;        /* 2*n_res undistorted pixel (unpx_ / runpx_)                 */
    const double *res_sigma;     /* n_res   2^scale                                            */
    const uint8_t *res_active;   /* n_res or NULL                                              */
    double calib_l[4], calib_r[4], T_rl[7];
} ov2_xyzba_problem;
typedef struct {
    double *poses_out;           /* 7*n_kf                                                     */
    double *xyz_out;             /* 3*n_pts                                                    */
    double *chi2_last_eval;      /* n_res, in/out like ov2_ba_result                           */
    uint8_t *depthpos_last_eval; /* n_res, in/out                                              */
    int iterations, num_successful_steps;
    double initial_cost, final_cost;
    int termination;             /* OV2_TERM_*                                                 */
    double solve_ms;
} ov2_xyzba_result;
int ov2_xyz_ba_solve(ov2_ctx *ctx, const ov2_xyzba_problem *p, const ov2_ba_options *o, ov2_xyzba_result *r);

/* ------------------------------------------------------------------ */
/* Per-keypoint undistortion + bearing vector                           */
/* ------------------------------------------------------------------ */
/* Frame::computeKeypoint (src/frame.cpp:246-254) for n keypoints in one launch:
 *   unpx = CameraCalibration::undistortImagePoint(px)   (src/camera_calibration.cpp:313-333:
 *          cv::undistortPoints(.., K, D, noArray(), K) for model pinhole, 5 iterations;
 *          cv::fisheye::undistortPoints(.., K, D, Mat(), K) for model fisheye; `return pt` when D is empty)
 *   bv   = normalize(iK * (unpx.x, unpx.y, 1))          (iK = the reference's K_.inverse(), row-major)
 * K = (fx, fy, cx, cy); D / nD = distortion coefficients (pinhole: 4, 5, 8 or 12; fisheye: 4; 0 = none).
 * px / unpx: n x (x,y) float; bv: n x 3 double, may be NULL.  The reference calls this per keypoint from
 * Frame::addKeypoint / updateKeypoint (src/frame.cpp:257-354) and for right-image points (:408).      */
#define OV2_CAM_PINHOLE 0
#define OV2_CAM_FISHEYE 1
int ov2_compute_keypoints(ov2_ctx *ctx, int model, const double K[4], const double *D, int nD, const double iK[9],
                          const float *px_xy_h, int n, float *unpx_xy_h, double *bv_xyz_h);
/* same on device-resident buffers (asynchronous on ctx's stream), e.g. straight on the output of ov2_fb_klt_d */
int ov2_compute_keypoints_d(ov2_ctx *ctx, int model, const double K[4], const double *D, int nD, const double iK[9],
                            const float *px_xy_d, int n, float *unpx_xy_d, double *bv_xyz_d);

/* ------------------------------------------------------------------ */
/* Stereo matching front half (MapManager::stereoMatching,              */
/* src/map_manager.cpp:367-611)                                         */
/* ------------------------------------------------------------------ */
/* FeatureTracker::getLineMinSAD (src/feature_tracker.cpp:138-206) for n keypoints in one launch, as called at
 * src/map_manager.cpp:431 on the coarsest pyramid level of a rectified pair: pts are ALREADY scaled to
 * `level` (kp.px_ * downpyrcoef), nwinsize odd (the reference uses 7), go_left = bgoleft.
 * xprior[i] = best column at that level or -1 (multiply by uppyrcoef like :433); l1err[i] = the minimal mean
 * absolute difference, 255 when nothing qualified (the reference leaves it unset on its early returns).
 * left/right: batch-1 pyramids of the two images (the image of `level` is read, REPLICATE border as
 * cv::getRectSubPix does); keypoints must lie inside that image.                                        */
int ov2_line_min_sad(ov2_ctx *ctx, const ov2_pyr *left, const ov2_pyr *right, int level, int nwinsize, int go_left,
                     const float *pts_xy_h, int n, float *xprior_h, float *l1err_h);
/* Epipolar gate of src/map_manager.cpp:568-590 for n (left keypoint, tracked right keypoint) pairs:
 *   runpx = pcalib_rightcam_->undistortImagePoint(rkps[i])        (model / K / D / nD as in ov2_compute_keypoints)
 *   rect != 0: epi_err = |lunpx.y - runpx.y| and rkps[i].y = lunpx[i].y (written back, :578)
 *   rect == 0: epi_err = MultiViewGeometry::computeSampsonDistance(Frl, lunpx, runpx)  (src/multi_view_geometry.cpp:797-822)
 *   ok[i] = epi_err <= 2.   runpx_xy_h / epi_err_h may be NULL.                                          */
int ov2_stereo_epipolar_check(ov2_ctx *ctx, int rect, const double Frl[9], int model, const double K[4], const double *D, int nD,
                              const float *lunpx_xy_h, float *rkps_xy_inout_h, int n, float *runpx_xy_h, float *epi_err_h, uint8_t *ok_h);

/* MapManager::stereoMatching's data path (src/map_manager.cpp:367-611) for the n keypoints of a keyframe in ONE enqueue and ONE
 * synchronisation (the three calls above need one each, plus a second fbKltTracking):
 *   rect != 0   getLineMinSAD on pyramid level nklt_pyr_lvl (window 7, searching left) gives the x prior of every keypoint
 *               without a 3-D prior when it lies in [0, kp.x] (:421-439)
 *   tracking    keypoints with has_prior3d_h[i] != 0 are tracked from priors3d_h[i] on 1 level first; the ones that fail join
 *               the second call with the first call's forward result as prior (:533-538: v3dpriors was updated in place); everything else runs on nklt_pyr_lvl levels (:544-565)
 *   gate        ov2_stereo_epipolar_check on the tracked right keypoints (model / K / D of the RIGHT camera, kps_unpx_h = the
 *               left keypoints' undistorted pixels)
 * Outputs: stereo_ok_h[i] (what decides updateKeypointStereo, :584) and right_px_h[i] (rect: y replaced by the left keypoint's,
 * :578; (0, 0) where the tracking itself failed -- a tracked point that the gate rejects keeps its position, stereo_ok 0).  has_prior3d_h / priors3d_h may be NULL (no map-point priors).  The right pyramid may
 * still be building on this context's stream (ov2_pyr_build_clahe_h is asynchronous).                                      */
int ov2_stereo_match(ov2_ctx *ctx, const ov2_pyr *left, const ov2_pyr *right, int nklt_win_size, int nklt_pyr_lvl, int max_iter,
                     float eps, float nklt_err, float fmax_fbklt_dist, int rect, const double Frl[9], int model, const double K[4],
                     const double *D, int nD, const float *kps_px_h, const float *kps_unpx_h, const float *priors3d_h,
                     const uint8_t *has_prior3d_h, int n, float *right_px_h, uint8_t *stereo_ok_h);

/* ov2_stereo_match for the keyframes of a lock-step batch (all sequences of a rank reach their keyframes together): items [0, n_items) of
 * two batch pyramids (left: e.g. ov2_btracker_cur_pyr at the keyframe; right: ov2_pyr_build_clahe_hb), n_max point slots per item
 * (item b's points are [b*n_max, b*n_max + n_h[b])), ONE enqueue and ONE synchronisation for all items -- the same kernels with the grid
 * extended by the item.  Per item the outputs equal ov2_stereo_match on that item.                                                */
int ov2_stereo_match_batch(ov2_ctx *ctx, const ov2_pyr *left, const ov2_pyr *right, int n_items, int nklt_win_size, int nklt_pyr_lvl, int max_iter,
                           float eps, float nklt_err, float fmax_fbklt_dist, int rect, const double Frl[9], int model, const double K[4],
                           const double *D, int nD, int n_max, const float *kps_px_h, const float *kps_unpx_h, const float *priors3d_h,
                           const uint8_t *has_prior3d_h, const int *n_h, float *right_px_h, uint8_t *stereo_ok_h);

/* ------------------------------------------------------------------ */
/* Keyframe triangulation (Mapper::triangulateStereo +                  */
/* Mapper::triangulateTemporal, src/mapper.cpp:191-461)                 */
/* ------------------------------------------------------------------ */
/* The mapper's two triangulation loops for a new keyframe (called back to back under map_mutex_, src/mapper.cpp:97, :120) in ONE
 * staging upload, ONE launch, ONE download and ONE synchronisation per call, one lane per keypoint in fp64 (csrc/triangulate.hip):
 *   stereo      keypoints with is_stereo[i] != 0 (the caller flags is_stereo_ && !is3d_ keypoints, :388-395):
 *               rect:  disp = unpx.x - runpx.x in float; disp < 0 rejects; z = (float)(K[0] |Tcic0.t| / fabs(disp));
 *                      left = z * iK * (unpx.x, unpx.y, 1)  (disp == 0 passes and gives a NaN point, accepted like the reference)
 *               else:  left = triangulate2(Tlr, bv, rbv)
 *               rejected if left.z < 0.1 or (Tlr^-1 left).z < 0.1, or if |proj_K(left) - unpx| or |proj_Kr(Tcic0 left) - runpx|
 *               exceeds fmax_reproj_err (cv::Point2f projections, cv::norm, float); otherwise wpt = Twc left, invdepth = 1 / left.z
 *   temporal    keypoints with src[i] >= 0 that the stereo pass did not make 3-D.  The host decides eligibility from the map
 *               (:243-295: the map point exists, is not 3-D, has >= 2 observers, its first observer ci is not this keyframe and
 *               holds the keypoint) and passes ci's row of the source table and ci's keypoint (src_unpx, src_bv):
 *               Tcicj = Tcw[ci] Twc; in stereo mode |Tcicj.t| < 0.01 skips (OV2_TRI_NO_MOTION); left = triangulate2(Tcicj,
 *               src_bv, bv), right = Tcicj^-1 left; the same depth and reprojection gates (left K on both sides); a rejection
 *               with rotation-compensated parallax > 20 px asks for removeMapPointObs; otherwise wpt = Twc[ci] left.
 * triangulate2 is OpenGV's closed-form midpoint (the USE_OPENGV build, src/multi_view_geometry.cpp:53-100, the one the paper's
 * results used); the OpenCV fallback (cv::triangulatePoints) is not provided.  Poses are [tx ty tz qx qy qz qw] taken as held by
 * the Frame / CameraCalibration (no renormalisation); the library inverts only where the reference does (Trl :379, Tcjci :280).
 * Status bits per keypoint (what a caller needs to replay every map mutation in the reference's order: the stereo keypoints in
 * order, then the temporal ones):
 *   STEREO_TRIED && !STEREO_OK   removeStereoKeypointById(lmid)
 *   STEREO_OK / TEMPORAL_OK      updateMapPoint(lmid, wpt, invdepth)   (anchor: this keyframe / the source keyframe)
 *   TEMPORAL_TRIED               counted in the reference's `candidates`
 *   NO_MOTION                    skipped, no mutation
 *   REMOVE_OBS                   removeMapPointObs(lmid, this keyframe's id)
 * wpt / invdepth are 0 where no point was created.  OV2_EINVAL: NULL ctx / params / buffers, n or n_src < 0, n_items < 0, a source
 * index outside [-1, n_src), a point flagged stereo without runpx / rbv or in mono mode, a temporal point without src_unpx /
 * src_bv; nothing is modified then.  */
enum {
    OV2_TRI_STEREO_TRIED = 1, OV2_TRI_STEREO_OK = 2, OV2_TRI_TEMPORAL_TRIED = 4, OV2_TRI_TEMPORAL_OK = 8,
    OV2_TRI_NO_MOTION = 16, OV2_TRI_REMOVE_OBS = 32
};
typedef struct {
    int stereo;                  /* pslamstate_->stereo_ (the no-motion skip, :287)                                          */
    int rect;                    /* bdo_stereo_rect_ (:410)                                                                  */
    float fmax_reproj_err;       /* fmax_reproj_err_                                                                         */
    double K[4];                 /* left fx fy cx cy (projCamToImage)                                                        */
    double iK[9];                /* left iK_, row-major (the rectified branch)                                               */
    double Kr[4];                /* right fx fy cx cy (projCamToRightImage)                                                  */
    double Tlr[7];               /* pcalib_rightcam_->getExtrinsic() (Tc0ci_)                                                */
    double Tcic0[7];             /* pcalib_rightcam_->Tcic0_ as held                                                         */
} ov2_tri_params;
typedef struct {
    int n;                       /* keypoints of the new keyframe                                                            */
    const double *Twc;           /* 7: the new keyframe's Twc_                                                               */
    const float *unpx;           /* 2n                                                                                       */
    const double *bv;            /* 3n                                                                                       */
    const uint8_t *is_stereo;    /* n or NULL (no stereo keypoint)                                                           */
    const float *runpx;          /* 2n, needed when a point is flagged stereo                                                */
    const double *rbv;           /* 3n, likewise                                                                             */
    const int *src;              /* n or NULL: row of the source table, -1 = no temporal candidate                           */
    const float *src_unpx;       /* 2n: the source keyframe's keypoint of the same map point (needed where src[i] >= 0)      */
    const double *src_bv;        /* 3n                                                                                       */
    int n_src;                   /* rows of the source table                                                                 */
    const double *src_Twc;       /* 7 n_src: Twc_ of each source keyframe                                                    */
    const double *src_Tcw;       /* 7 n_src: Tcw_ of each source keyframe, as held                                           */
} ov2_tri_keyframe;
typedef struct {
    uint8_t *status;             /* n: OV2_TRI_* bits                                                                        */
    double *wpt;                 /* 3n                                                                                       */
    double *invdepth;            /* n                                                                                        */
    int n_stereo, n_stereo_good; /* the reference's nbstereo / good of the stereo pass                                       */
    int n_candidates, n_temporal_good;   /* candidates / good of the temporal pass                                           */
} ov2_tri_result;
/* one keyframe: the batch form with one item, through the same code path */
int ov2_triangulate_keyframe(ov2_ctx *ctx, const ov2_tri_params *params, const ov2_tri_keyframe *kf, ov2_tri_result *result);
/* the keyframes of a lock-step batch, items [0, n_items) with shared params (one grid, grid.y = item; n_items <= 65535, else
 * OV2_EUNSUPPORTED).  Per item the result equals ov2_triangulate_keyframe on that item; an item with n == 0 is allowed. */
int ov2_triangulate_keyframe_batch(ov2_ctx *ctx, const ov2_tri_params *params, int n_items, const ov2_tri_keyframe *kfs,
                                   ov2_tri_result *results);

/* ------------------------------------------------------------------ */
/* Local-map matching (Mapper::matchToMap, src/mapper.cpp:576-774)      */
/* ------------------------------------------------------------------ */
/* The loop that Mapper::matchingToLocalMap runs after the triangulation: every 3-D point of the local map is projected into the
 * new keyframe and compared, by descriptor, with the map points of the keypoints around its projection; a match says "this
 * keypoint's map point is a re-detection of that local map point" (mergeMatches).  One wavefront per local map point
 * (csrc/mapmatch.hip), ONE staging upload, the launches, ONE download and ONE synchronisation per call.
 *
 * Thresholds, once per call on the host in float as the reference writes them: vfov = 0.5 img_h / fy, hfov = 0.5 img_w / fx,
 * view_th = cos(atan(max(hfov, vfov))); dmaxpxdist = fmax_proj_pxdist, doubled when nb3dkps < 30; mindist = (float)(desc_bytes *
 * fmax_desc_dist * 8.).
 * Per local map point l, in the caller's order, with wpt = lm_wpt[l] and A = lm_mp[l] (its row of the map-point table):
 *   campt = Tcw wpt (Sophus SE3d * Vector3d, the pose as held); campt.z < 0.1 -> BEHIND; view_angle = (float)(campt.z / |campt|),
 *   fabs(view_angle) < view_th -> OUT_OF_FOV; projpx = projectCamToImageDist(campt) (below); outside [0, img_w) x [0, img_h) (or
 *   NaN) -> OUT_OF_IMAGE.
 *   Candidates: the keypoints of cells r in {rkp-1, rkp}, c in {ckp-1, ckp}, rkp = floor(projpx.y / ncellsize), ckp alike (a 2x2
 *   block as the reference's loop bounds give it, not 3x3; r < 0 or c < 0 skipped), cell index r * ceil(img_w / ncellsize) + c, in
 *   that order and inside a cell in the order of cell_kp.  A candidate keypoint k with B = kp_mp[k] >= 0 and B holding a descriptor:
 *     pxdist = (float)cv::norm(projpx - kp_px[k]) > dmaxpxdist                       -> skipped
 *     A and B share an observing keyframe id (obs_kfid; stale observations count)     -> skipped
 *     coprojpx (float) += cv::norm(obs_px - projWorldToImageDist_kf(wpt)) over B's observations with obs_kf >= 0, in ascending
 *     keyframe id; coprojpx / count > dmaxpxdist -> skipped (count == 0: NaN, the candidate passes; no depth check here)
 *     dist = the minimum Hamming distance over all (descriptor of A, descriptor of B) pairs, start value 1000
 *     dist <= bestdist: best -> second, k -> best;  else dist <= secdist: k -> second   (both start at mindist, id -1)
 *   best and second both set and 0.9 * secdist < bestdist -> RATIO_REJECTED; no best -> NO_CANDIDATE; otherwise BEST: the point
 *   proposes keypoint lm_kp[l] at lm_dist[l].
 * Per keypoint the proposing point with the smallest distance wins, among equals the one listed LAST in the local map (the
 * reference's `<=`): kp_lm[k] / kp_dist[k]; kp_lm is the reference's map_previd_newid as (keypoint row -> local-map index).
 * The pick is a 64-bit atomic minimum on (distance, reversed index), so a call's bytes do not depend on scheduling.
 * lm_projpx is (0, 0) for BEHIND / OUT_OF_FOV points; lm_dist is the final bestdist (mindist when nothing qualified) and 0 for
 * points that a gate removed; lm_kp is -1 unless BEST.
 *
 * projectCamToImageDist (src/camera_calibration.cpp:254-281): x = X / z, y = Y / z in double through invz = 1 / z; nD == 0:
 * Point2f(fx x + cx, fy y + cy).  Otherwise x, y are first rounded to float (cv::Point3f / Point2f) and run, in double, through
 * cv::projectPoints with zero rotation and translation (OV2_CAM_PINHOLE, k1 k2 p1 p2 [k3 [k4 k5 k6 [s1 s2 s3 s4]]], nD = 4 / 5 / 8
 * / 12) or cv::fisheye::distortPoints (OV2_CAM_FISHEYE, nD = 4); the result is rounded to float.  Both are restated from the
 * published models, not pinned against an OpenCV build.
 *
 * What stays on the host: choosing the local map, the filters that need the map's hash tables (isObservingKp, missing / 2-D /
 * descriptor-less points, :613-623), mergeMatches, and the map clean-up the reference does in passing (:678-681, :708-713).
 * DEVIATION (snapshot): the caller marks a stale observation (its keyframe is gone or no longer holds the keypoint) with
 * obs_kf = -1 when it flattens the map.  Such an observation still counts in the shared-observer test and is left out of the
 * re-projection sum, as in the reference the first time it is met; the reference then removes it from the map, so a LATER local
 * map point of the same call would see the cleaned set.  Without stale observations the two agree exactly.
 *
 * OV2_EINVAL: NULL params / keyframe / result / ctx, a negative count, a NULL array with a non-zero count, kp_mp / lm_mp / obs_kf
 * / cell_kp outside its table, offsets (cell_start, obs_start, desc_start) that do not start at 0 or decrease, obs_kfid not strictly
 * ascending inside a row, img_w / img_h / ncellsize not positive.  OV2_EUNSUPPORTED: desc_bytes != 32, a coefficient count the model
 * does not take, more than 65535 items, more than 2^31 - 1 elements of one kind in a call.  All of it is checked on the host
 * before any device work (the inputs before the context, so a malformed input is reported without a device); nothing is
 * modified then. */
enum {
    OV2_MATCH_BEHIND = 1, OV2_MATCH_OUT_OF_FOV = 2, OV2_MATCH_OUT_OF_IMAGE = 4, OV2_MATCH_NO_CANDIDATE = 8,
    OV2_MATCH_RATIO_REJECTED = 16, OV2_MATCH_BEST = 32
};
typedef struct {
    int model;                   /* OV2_CAM_PINHOLE / OV2_CAM_FISHEYE                                                        */
    double K[4];                 /* fx fy cx cy                                                                              */
    const double *D;             /* nD distortion coefficients (NULL when nD == 0)                                           */
    int nD;
    double img_w, img_h;         /* pcalib_leftcam_->img_w_ / img_h_                                                         */
    int ncellsize;               /* Frame::ncellsize_                                                                        */
    float fmax_proj_pxdist;      /* fmaxprojerr                                                                              */
    float fmax_desc_dist;        /* fdistratio                                                                               */
    int desc_bytes;              /* desc_.cols: 32                                                                           */
} ov2_match_params;
typedef struct {
    const double *Tcw;           /* 7: the keyframe's Tcw_ as held                                                           */
    int nb3dkps;                 /* frame.nb3dkps_                                                                           */
    int n_kp;                    /* keypoints                                                                                */
    const float *kp_px;          /* 2 n_kp: px_                                                                              */
    const int *kp_mp;            /* n_kp: row of the map-point table, -1 = no usable map point                               */
    const int *cell_start;       /* ncells + 1 offsets into cell_kp, ncells = ceil(img_w / ncellsize) * ceil(img_h / ncellsize) */
    const int *cell_kp;          /* keypoint rows, per cell in vgridkps_ order                                               */
    int n_mp;                    /* rows of the map-point table (local map points and the keypoints' map points alike)       */
    const int *obs_start;        /* n_mp + 1                                                                                 */
    const int *obs_kfid;         /* per observation: keyframe id, strictly ascending inside a row                            */
    const int *obs_kf;           /* per observation: row of the pose table, -1 = stale                                       */
    const float *obs_px;         /* 2 per observation: the observing keyframe's px_ of that map point                        */
    const int *desc_start;       /* n_mp + 1                                                                                 */
    const uint8_t *desc;         /* desc_bytes per descriptor: the map point's map_kf_desc_, any order                       */
    int n_kf;                    /* rows of the pose table                                                                   */
    const double *kf_Tcw;        /* 7 n_kf, as held                                                                          */
    int n_lm;                    /* local map points, in the caller's iteration order                                        */
    const int *lm_mp;            /* n_lm: row of the map-point table                                                         */
    const double *lm_wpt;        /* 3 n_lm                                                                                   */
} ov2_match_keyframe;
typedef struct {
    uint8_t *lm_status;          /* n_lm: OV2_MATCH_* bits                                                                   */
    int *lm_kp;                  /* n_lm: proposed keypoint row or -1                                                        */
    float *lm_dist;              /* n_lm                                                                                     */
    float *lm_projpx;            /* 2 n_lm                                                                                   */
    int *kp_lm;                  /* n_kp: the winning local-map index or -1                                                  */
    float *kp_dist;              /* n_kp: its distance (0 where kp_lm == -1)                                                 */
    int n_matches;               /* keypoints with kp_lm >= 0                                                                */
} ov2_match_result;
/* one keyframe: the batch form with one item, through the same code path */
int ov2_match_to_map(ov2_ctx *ctx, const ov2_match_params *params, const ov2_match_keyframe *kf, ov2_match_result *result);
/* the keyframes of a lock-step batch, items [0, n_items) with shared params (grid.y = item).  Per item the result equals
 * ov2_match_to_map on that item; an item without local map points or without keypoints is allowed. */
int ov2_match_to_map_batch(ov2_ctx *ctx, const ov2_match_params *params, int n_items, const ov2_match_keyframe *kfs,
                           ov2_match_result *results);

/* ------------------------------------------------------------------ */
/* Descriptor kNN matching (LoopCloser::knnMatching,                    */
/* src/loop_closer.cpp:378-459)                                         */
/* ------------------------------------------------------------------ */
/* The first stage of LoopCloser::processLoopCandidate: cv::BFMatcher(cv::NORM_HAMMING).knnMatch(query, train, vmatches, 2) and
 * the loop :432-449 that keeps a query row when it has fewer than two neighbours, or when d0 <= maxdist && d0 <= d1 * 0.85.  One
 * lane per query row (csrc/knn.hip); ONE staging upload, the launches, ONE download and ONE synchronisation per call.  A call with
 * few items and many train rows spreads ranges of train rows over more work-groups and merges their candidates on the device;
 * the order-free definition below makes the result the same bytes either way.
 *
 * Per query row q the two neighbours are the two smallest (Hamming distance, train row) pairs in lexicographic order: among equal
 * distances the lower train row comes first, which is what OpenCV's batchDistance produces by visiting the train rows in ascending
 * order with strict comparisons.  idx[2q], idx[2q+1] are their train rows (-1: no such neighbour), dist[2q], dist[2q+1] their
 * distances as int (what DMatch::distance holds as a float; -1 where idx is -1).
 *   good[q] = idx0 >= 0 && (idx1 < 0 || (d0 <= max_dist && (double)d0 <= (double)d1 * ratio))     (fp64, no contraction)
 * so a train set of ONE row makes every query good whatever its distance (the reference's m.size() < 2), and an empty train set
 * or an empty query set gives no pairs (the reference returns before it matches, :422-424).  There is no cross-check: several
 * queries may take the same train row.  pair_query / pair_train list (q, idx0) of the good rows in query order, n_pairs of them:
 * the reference appends (vkpids[q], vlmids[idx0]) for exactly these.  The reference's settings are desc_bytes = 32,
 * max_dist = (int)(desc_bytes * 0.5 * 8.) = 128, ratio = 0.85.
 * BFMatcher::knnMatch is restated from OpenCV's published source, not pinned against an OpenCV build.
 *
 * What stays on the host: the two frame walks that collect the rows and their ids (:391-420).
 *
 * OV2_EINVAL: NULL params / item / result / ctx, a negative count, a NULL array with a non-zero count, max_dist < 0, ratio negative
 * or not finite.  OV2_EUNSUPPORTED: desc_bytes != 32, more than 65535 items, more than 2^31 - 1 query or train rows in a call.
 * All of it is checked on the host before any device work (the inputs before the context, so a malformed input is reported
 * without a device); nothing is modified then. */
typedef struct {
    int desc_bytes;              /* query.cols: 32                                                                           */
    int max_dist;                /* maxdist: (int)(desc_bytes * 0.5 * 8.)                                                    */
    double ratio;                /* 0.85                                                                                     */
} ov2_knn_params;
typedef struct {
    int n_query, n_train;
    const uint8_t *query;        /* desc_bytes per row                                                                       */
    const uint8_t *train;
} ov2_knn_item;
typedef struct {
    int *idx;                    /* 2 n_query: train rows of the nearest and the second nearest, -1 = none                   */
    int *dist;                   /* 2 n_query: their Hamming distances, -1 where idx is -1                                   */
    uint8_t *good;               /* n_query                                                                                  */
    int *pair_query;             /* capacity n_query: the good query rows, ascending                                         */
    int *pair_train;             /* capacity n_query: their nearest train rows                                               */
    int n_pairs;
} ov2_knn_result;
/* one query / train pair: the batch form with one item, through the same code path */
int ov2_knn_match(ov2_ctx *ctx, const ov2_knn_params *params, const ov2_knn_item *item, ov2_knn_result *result);
/* items [0, n_items) with shared params (grid.y = item).  Per item the result equals ov2_knn_match on that item; an item with
 * n_query == 0 or n_train == 0 is allowed and has n_pairs = 0. */
int ov2_knn_match_batch(ov2_ctx *ctx, const ov2_knn_params *params, int n_items, const ov2_knn_item *items, ov2_knn_result *results);

/* ------------------------------------------------------------------ */
/* Loop local-map tracking (LoopCloser::trackLoopLocalMap /             */
/* LoopCloser::matchToMap, src/loop_closer.cpp:502-763)                 */
/* ------------------------------------------------------------------ */
/* The fourth stage of LoopCloser::processLoopCandidate: once P3P has put the new keyframe into the loop keyframe's frame, the 3-D
 * points of the loop keyframe's neighbourhood are projected into the new keyframe and matched, by descriptor, with the map points
 * of the keypoints around their projections.  A cousin of ov2_match_to_map with other gates and other arithmetic -- a different
 * function of the reference, not a mode of that one.  One wavefront per local map point (csrc/mapmatch.hip), ONE staging upload,
 * two launches, ONE download and ONE synchronisation per call.
 *
 * Thresholds, once per call on the host in float as the reference writes them (:595-607, :656): hfov = (float)(0.5 * img_w * fx)
 * -- MULTIPLIED by the focal length, and atan(hfov) in both branches of the reference's `if`, so vfov is never used --,
 * view_th = (float)cos((float)atan(hfov)), each step taken in double and rounded to float (EuRoC: 5.797544e-06, i.e. the cone
 * removes next to nothing); dmaxpxdist = fmax_proj_pxdist as given (the reference passes 10.); mindist = (float)(desc_bytes *
 * fmax_desc_dist * 8.) (the reference passes fmax_desc_dist_ * 1.5 as a float).
 * Per local map point l, in the caller's order, with wpt = lm_wpt[l] and A = lm_mp[l] (its row of the map-point table):
 *   campt = Tcw wpt (Sophus SE3d * Vector3d; Tcw is the caller's Twc.inverse(), the P3P / PnP result, not the frame's pose);
 *   campt.z < 0.1 -> BEHIND; view_angle = (float)(campt.z / |campt|), fabs(view_angle) < view_th -> OUT_OF_FOV; projpx =
 *   projectCamToImageDist(campt) (as for ov2_match_to_map); outside [0, img_w) x [0, img_h) (or NaN) -> OUT_OF_IMAGE.
 *   Candidates: the keypoints of cells r in {rkp-1, rkp}, c in {ckp-1, ckp}, rkp = floor(projpx.y / ncellsize), ckp alike (the 2x2
 *   block of Frame::getSurroundingKeypoints(cv::Point2f); r < 0 or c < 0 skipped), cell index r * ceil(img_w / ncellsize) + c, in
 *   that order and inside a cell in the order of cell_kp.  A candidate keypoint k is skipped when
 *     kp_matched[k] != 0 (its lmid_ is in vmatchedkpids, :672-675), or kp_mp[k] < 0 or B = kp_mp[k] holds no descriptor, or
 *     pxdist = (float)cv::norm(projpx - kp_px[k]) > dmaxpxdist, or
 *     A and B share an observing keyframe id (obs_kfid).
 *   Otherwise dist = the minimum Hamming distance over all (descriptor of A, descriptor of B) pairs, start value 1000;
 *     dist <= bestdist: best -> second, k -> best;  else dist <= secdist: k -> second   (both start at mindist, id -1)
 *   best and second both set and 0.9 * secdist < bestdist -> RATIO_REJECTED; no best -> NO_CANDIDATE; otherwise BEST: the point
 *   proposes keypoint lm_kp[l] at lm_dist[l].
 * There is no re-projection into the candidate's observers, no pose table, and the loop only reads the map: the flat form and the
 * reference agree without any deviation.
 * Per keypoint the proposing point with the smallest distance wins, among equals the one listed LAST in the local map (the
 * reference's `<=`): kp_lm[k] / kp_dist[k]; kp_lm is the reference's map_previd_newid as (keypoint row -> local-map index).
 * The pick is a 64-bit atomic minimum on (distance, reversed index), so a call's bytes do not depend on scheduling.
 * lm_projpx is (0, 0) for BEHIND / OUT_OF_FOV points; lm_dist is the final bestdist (mindist when nothing qualified) and 0 for
 * points that a gate removed; lm_kp is -1 unless BEST.
 *
 * What stays on the host: the covisible-keyframe walk that builds the local set and vmatchedkpids (:505-562; ov2slam_amd/host/
 * loop_closer.hpp has it as loopLocalMapReferenceOrder), the filters that need the map's hash tables (isObservingKp, missing / 2-D
 * / bad / descriptor-less points, :614-631), and appending the matches to vkplmids (:576-582).
 *
 * OV2_EINVAL: NULL params / item / result / ctx, a negative count, a NULL array with a non-zero count, kp_mp / lm_mp / cell_kp
 * outside its table, offsets (cell_start, obs_start, desc_start) that do not start at 0 or decrease, obs_kfid not strictly
 * ascending inside a row, img_w / img_h / ncellsize not positive.  OV2_EUNSUPPORTED: desc_bytes != 32, a coefficient count the model
 * does not take, more than 65535 items, more than 2^31 - 1 elements of one kind in a call.  All of it is checked on the host
 * before any device work (the inputs before the context, so a malformed input is reported without a device); nothing is
 * modified then. */
enum {
    OV2_LOOPMAP_BEHIND = 1, OV2_LOOPMAP_OUT_OF_FOV = 2, OV2_LOOPMAP_OUT_OF_IMAGE = 4, OV2_LOOPMAP_NO_CANDIDATE = 8,
    OV2_LOOPMAP_RATIO_REJECTED = 16, OV2_LOOPMAP_BEST = 32
};
typedef struct {
    int model;                   /* OV2_CAM_PINHOLE / OV2_CAM_FISHEYE                                                        */
    double K[4];                 /* fx fy cx cy                                                                              */
    const double *D;             /* nD distortion coefficients (NULL when nD == 0)                                           */
    int nD;
    double img_w, img_h;         /* pcalib_leftcam_->img_w_ / img_h_                                                         */
    int ncellsize;               /* Frame::ncellsize_                                                                        */
    float fmax_proj_pxdist;      /* fmaxprojerr: the reference passes 10.                                                    */
    float fmax_desc_dist;        /* fdistratio: the reference passes fmax_desc_dist_ * 1.5                                   */
    int desc_bytes;              /* desc_.cols: 32                                                                           */
} ov2_loopmap_params;
typedef struct {
    const double *Tcw;           /* 7: Twc.inverse() of the P3P / PnP result                                                 */
    int n_kp;                    /* keypoints of the new keyframe                                                            */
    const float *kp_px;          /* 2 n_kp: px_                                                                              */
    const int *kp_mp;            /* n_kp: row of the map-point table, -1 = no usable map point                               */
    const uint8_t *kp_matched;   /* n_kp: non-zero = the keypoint's lmid_ is in vmatchedkpids                                */
    const int *cell_start;       /* ncells + 1 offsets into cell_kp, ncells = ceil(img_w / ncellsize) * ceil(img_h / ncellsize) */
    const int *cell_kp;          /* keypoint rows, per cell in vgridkps_ order                                               */
    int n_mp;                    /* rows of the map-point table (local map points and the keypoints' map points alike)       */
    const int *obs_start;        /* n_mp + 1                                                                                 */
    const int *obs_kfid;         /* per observation: keyframe id, strictly ascending inside a row                            */
    const int *desc_start;       /* n_mp + 1                                                                                 */
    const uint8_t *desc;         /* desc_bytes per descriptor: the map point's map_kf_desc_, any order                       */
    int n_lm;                    /* local map points, in the caller's iteration order                                        */
    const int *lm_mp;            /* n_lm: row of the map-point table                                                         */
    const double *lm_wpt;        /* 3 n_lm                                                                                   */
} ov2_loopmap_item;
typedef struct {
    uint8_t *lm_status;          /* n_lm: OV2_LOOPMAP_* bits                                                                 */
    int *lm_kp;                  /* n_lm: proposed keypoint row or -1                                                        */
    float *lm_dist;              /* n_lm                                                                                     */
    float *lm_projpx;            /* 2 n_lm                                                                                   */
    int *kp_lm;                  /* n_kp: the winning local-map index or -1                                                  */
    float *kp_dist;              /* n_kp: its distance (0 where kp_lm == -1)                                                 */
    int n_matches;               /* keypoints with kp_lm >= 0                                                                */
} ov2_loopmap_result;
/* one loop candidate: the batch form with one item, through the same code path */
int ov2_loop_match_to_map(ov2_ctx *ctx, const ov2_loopmap_params *params, const ov2_loopmap_item *item, ov2_loopmap_result *result);
/* items [0, n_items) with shared params (grid.y = item).  Per item the result equals ov2_loop_match_to_map on that item; an item
 * without local map points or without keypoints is allowed. */
int ov2_loop_match_to_map_batch(ov2_ctx *ctx, const ov2_loopmap_params *params, int n_items, const ov2_loopmap_item *items,
                                ov2_loopmap_result *results);

/* ------------------------------------------------------------------ */
/* Loop-closure keyframe preparation (LoopCloser::run,                  */
/* src/loop_closer.cpp:86-144)                                          */
/* ------------------------------------------------------------------ */
/* What LoopCloser::run does with every new keyframe before the place recogniser sees it: a mask that is 255 everywhere with a
 * cv::circle(mask, kp.px_, 2., 0, -1) at each keypoint whose map point already has a descriptor, FastFeatureDetector::create(20)
 * ->detect on the whole raw left image under that mask, KeyPointsFilter::retainBest(vaddkps, 300), and BriefDescriptorExtractor::
 * compute on what is left.  Integers throughout; every output is the same bytes whatever the call form and from run to run.
 * Per item: a u8 image w x h, n_excl float points excl_xy (x, y), and the parameters below.
 *   1 FAST    cv::FAST(img, threshold, nonmaxSuppression = true, TYPE_9_16).  threshold is clamped to [0, 255].  Candidates are
 *             3 <= x < w-3, 3 <= y < h-3 (none when w < 7 or h < 7); a candidate is a corner when 9 contiguous pixels of its
 *             16-pixel ring are all < v - threshold or all > v + threshold; its score is cornerScore<16>.  A corner survives when
 *             its score is strictly greater than the scores of its eight neighbours (not a corner / outside the candidate range:
 *             0).  The response is the score, 1 .. 255.
 *   2 mask    a corner at (x, y) is dropped when the filled circle of some exclusion point covers the pixel: centre
 *             (rint(px), rint(py)) (half to even), radius excl_radius, OpenCV's midpoint circle clipped to the image -- the pixels
 *             ov2_set_mask paints.  A point with a non-finite coordinate paints nothing.
 *   3 retain  KeyPointsFilter::retainBest(retain): retain < 0 keeps every corner, retain == 0 none; at most `retain` corners
 *             left: all are kept (cut = 0); otherwise cut = the retain-th largest response and EVERY corner with response >= cut
 *             is kept (std::nth_element + std::partition(>= ambiguous_response) as a set): ties at the cut are the normal case,
 *             so n_kept > retain is.
 *   4 BRIEF   compute() first removes keypoints outside [28, w-28) x [28, h-28) (runByImageBorder) -- AFTER retainBest, so fewer
 *             than `retain` descriptors is normal -- and describes the rest with the context's pattern, exactly as
 *             ov2_describe_brief does on the same image and integer points: kept_valid is that call's valid, kept_desc its rows
 *             (32 zero bytes where valid == 0).
 *   5 order   both lists are in raster order (y ascending, then x).  The reference's order is whatever libstdc++'s nth_element /
 *             partition leave: a permutation of the same set (ov2slam_amd/host/loop_closer.hpp reproduces it on the host).
 * Truncation is not an error: a list is cut at its capacity in raster order, the counts stay the true ones, and a slot's
 * descriptor is written only when the slot exists.  Slots past min(count, capacity) are not written.
 *
 * What stays on the host: the frame walk that collects the exclusion points and the existing descriptors, and the cv::vconcat
 * of the two descriptor sets.  The ORB fallback of a build without OPENCV_CONTRIB (cv::ORB::create(500, 1., 0)) is not covered.
 * cv::FAST, KeyPointsFilter and BriefDescriptorExtractor::compute restated from OpenCV's published source, not pinned against an
 * OpenCV build.
 *
 * The host forms do ONE staging upload, the launches, ONE download and ONE synchronisation.  Device scratch per item (the
 * context's grow-only buffer): a u8 score map (w rounded up to 64, times h), a bit mask (w / 8 bytes per row), 16 B per row, a
 * 1 KB histogram and 8 B per kept slot; the batch forms walk the items in chunks that fit OV2_OPT_LCKF_SCRATCH_KB (same bytes
 * whatever the chunk size; still one synchronisation).
 *
 * OV2_EINVAL: a NULL argument (a list pointer may be NULL when its capacity or count is 0), a negative count or capacity,
 * w or h < 1, stride < w, item_stride smaller than one image, excl_radius outside [0, 64] (the half-width table of the painter).
 * OV2_EUNSUPPORTED: an image side of 2^15 or more (int16 coordinates), more than 65535 items.  All of it is checked on the host,
 * the inputs before the context or the tracker's state; nothing is written then. */
typedef struct { int threshold, retain, excl_radius; } ov2_lckf_params;      /* reference: 20, 300, 2 */
int ov2_lckf_params_init(ov2_lckf_params *out);
typedef struct {
    int n_all;            /* corners after NMS and mask filter (true count, may exceed all_cap)           */
    int cut;              /* the retain-th largest response, 0 when nothing was cut                        */
    int n_kept;           /* retained corners (true count, may exceed kept_cap)                            */
    int n_desc;           /* of those, inside the BRIEF border (valid == 1)                                */
    int16_t *all_xy; uint8_t *all_resp; int all_cap;      /* optional (NULL / 0): the pre-retain list, raster order */
    int16_t *kept_xy; uint8_t *kept_resp; uint8_t *kept_valid; uint8_t *kept_desc; int kept_cap;  /* 32 B per slot */
} ov2_lckf_result;
/* host image (w x h, rows `stride` bytes apart), n_excl host points (x, y) */
int ov2_lckf_prepare(ov2_ctx *ctx, const uint8_t *img_h, int w, int h, int stride, const ov2_lckf_params *params,
                     const float *excl_xy_h, int n_excl, ov2_lckf_result *result);
/* the RAW frame of the tracker's current frame, the one ov2_tracker_describe_brief reads: no image upload */
int ov2_tracker_lckf_prepare(ov2_tracker *t, const ov2_lckf_params *params, const float *excl_xy_h, int n_excl,
                             ov2_lckf_result *result);
/* n_items device images `item_stride` bytes apart (rows `pitch` bytes apart); device exclusion points, excl_cap slots per item,
 * n_excl_d[b] of them valid (counts above excl_cap are taken as excl_cap; n_excl_d may be NULL when excl_cap == 0); device outputs
 * in slot layouts: all_* all_cap slots per item (may be NULL / 0), kept_* kept_cap slots per item, counts_d 4 ints per item
 * {n_all, cut, n_kept, n_desc}.  Synchronises once. */
int ov2_lckf_prepare_batch_d(ov2_ctx *ctx, const ov2_lckf_params *params, const uint8_t *img_d, int w, int h, int pitch,
                             size_t item_stride, int n_items, const float *excl_xy_d, int excl_cap, const int *n_excl_d,
                             int16_t *all_xy_d, uint8_t *all_resp_d, int all_cap, int16_t *kept_xy_d, uint8_t *kept_resp_d,
                             uint8_t *kept_valid_d, uint8_t *kept_desc_d, int kept_cap, int *counts_d);
/* the raw frames of the current lock-step step, items [0, n_active): host exclusion points with excl_cap slots per item
 * (n_excl_h[b] valid), one result per item (capacities may differ).  OV2_EINVAL once the staging set that held those frames has
 * been uploaded or prepared again, as for ov2_btracker_describe_brief: in the look-ahead loop, call right after the step. */
int ov2_btracker_lckf_prepare(ov2_btracker *t, int n_active, const ov2_lckf_params *params, const float *excl_xy_h,
                              const int *n_excl_h, int excl_cap, ov2_lckf_result *results);

/* ==================================================================== */
/* Absolute pose from 2D-3D matches (MultiViewGeometry::p3pRansac,      */
/* src/multi_view_geometry.cpp:144-343, USE_OPENGV)                     */
/* ==================================================================== */
/* What VisualFrontEnd::computePose runs when the motion model is wrong (the p3p_req of the trackers) and what the loop closer
 * runs per candidate: Kneip's P3P on three matches of a sample row, the row's fourth match picks among its solutions, and the
 * hypotheses are searched as OpenGV's sac::Lmeds (smallest median of sqrt(1 - cos)) or sac::Ransac (largest inlier count, adaptive
 * iteration bound) would.  fp64 (csrc/p3p.hip): ONE staging upload, three launches, ONE download, ONE synchronisation per call.
 *
 * The sample table is an INPUT (n_rows x 4 indices), so the result is a deterministic function of the arguments: hypotheses are
 * evaluated in parallel, the winner is chosen exactly as the sequential loop over the rows in order would choose it.  A row with
 * a repeated or out-of-range index, without a solution (an accepted root of the quartic whose pose reproduces the row's own
 * three bearings to d <= 1e-12) or with a non-finite model is skipped WITHOUT counting an
 * iteration; the search stops when its loop ends or the rows run out.  ov2_p3p_draw_samples fills a table (a caller draws
 * 2 x max_iterations rows so that skipped rows do not shorten the search).
 *   LMedS   while iterations < max_iterations: a strictly smaller penalty becomes the best; ++iterations.  The penalty is the exact
 *           median of sqrt(d): sqrt(d[n/2]) for odd n, the mean of the two middle square roots for even n.
 *   RANSAC  k = 1; while iterations < k: a strictly larger inlier count (d < threshold) becomes the best and sets
 *           k = log(1 - probability) / log(1 - (count / n)^4) (the argument clamped to [DBL_EPSILON, 1 - DBL_EPSILON]); ++iterations;
 *           stop once iterations > max_iterations.
 * d_i = max(0, 1 - bv_i . v / |v|), v = Rwc^T (X_i - twc).  After either loop the outliers of the best model are the points with
 * d_i >= threshold, ascending.  The full specification is tests/p3p_ref.py; OpenGV itself is not available to this project, so the
 * solver and the loops are restated and nothing is pinned against an OpenGV binary.
 *
 * status: OV2_P3P_TOO_FEW_POINTS (n < 4: nothing else is set or searched), OV2_P3P_NO_MODEL (no valid row was reached; comes with
 * OV2_P3P_FEW_INLIERS), OV2_P3P_FEW_INLIERS (fewer than 5), OV2_P3P_NOT_ORTHOGONAL (Sophus::isOrthogonal fails on Rwc).  The
 * reference returns false on any of them.  model, score, best_row and the outlier list describe the best model whenever there is
 * one (best_row >= 0), whatever the status; without one they are 0 / -1 / empty.
 *
 * Capacity: OV2_P3P_MAX_POINTS points and OV2_P3P_MAX_ROWS rows per problem, 65535 problems per call.  OV2_EINVAL: NULL params /
 * problem / result / ctx, a NULL array with a non-zero count, a negative count, a non-finite bearing or point, threshold <= 0 or
 * not finite, probability outside (0, 1), max_iterations < 0, an unknown mode, boptimize != 0 (OpenGV's non-linear refinement is
 * not provided: refine with ov2_ba_solve / ov2::ceresPnP, as LoopCloser::computePnP does right after), anything beyond the
 * capacity.  All of it is checked on the host before any device work, the inputs before the context. */
enum { OV2_P3P_LMEDS = 0, OV2_P3P_RANSAC = 1 };
enum { OV2_P3P_TOO_FEW_POINTS = 1, OV2_P3P_NO_MODEL = 2, OV2_P3P_FEW_INLIERS = 4, OV2_P3P_NOT_ORTHOGONAL = 8 };
#define OV2_P3P_MAX_POINTS 2048
#define OV2_P3P_MAX_ROWS 4096
typedef struct {
    int mode;                    /* OV2_P3P_LMEDS / OV2_P3P_RANSAC                                                            */
    int max_iterations;          /* nmaxiter                                                                                 */
    double threshold;            /* 1 - cos(atan(errth / focal))                                                             */
    double probability;          /* 0.99                                                                                     */
    int boptimize;               /* must be 0                                                                                */
} ov2_p3p_params;
typedef struct {
    int n;                       /* matches                                                                                  */
    const double *bv;            /* 3 n: unit bearing vectors, camera frame                                                  */
    const double *X;             /* 3 n: world points                                                                        */
    int n_rows;                  /* rows of the sample table                                                                 */
    const int *samples;          /* 4 n_rows                                                                                 */
} ov2_p3p_problem;
typedef struct {
    double model[12];            /* Rwc row-major (9), twc (3)                                                               */
    double score;                /* the best row's penalty (LMedS) or inlier count (RANSAC)                                  */
    int best_row;                /* -1: no model                                                                             */
    int iterations;              /* rows that counted                                                                        */
    int rows_consumed;           /* rows the loop took from the table, skipped ones included                                 */
    int status;                  /* OV2_P3P_* bits, 0 = the reference returns true                                           */
    int n_inliers, n_outliers;
    int *outliers;               /* n slots; the first n_outliers are written, ascending                                     */
    uint8_t *trace_valid;        /* optional (NULL or n_rows): 1 where the row gave a hypothesis                             */
    double *trace_score;         /* optional (NULL or n_rows): every row's penalty or count, 0 for an invalid row            */
} ov2_p3p_result;
/* one problem: the batch form with one item, through the same code path */
int ov2_p3p_ransac(ov2_ctx *ctx, const ov2_p3p_params *params, const ov2_p3p_problem *problem, ov2_p3p_result *result);
/* the problems of a lock-step batch, items [0, n_items) with shared params (the problem is a grid axis: each kernel is launched
 * once).  Per item the result equals ov2_p3p_ransac on that item bit for bit; sizes may differ, empty problems are allowed. */
int ov2_p3p_ransac_batch(ov2_ctx *ctx, const ov2_p3p_params *params, int n_items, const ov2_p3p_problem *problems,
                         ov2_p3p_result *results);
/* Host only: rows x 4 indices of [0, n), distinct inside a row.  Draw j of the stream is splitmix64's output for the state
 * seed + (j + 1) * 0x9E3779B97F4A7C15, reduced modulo n; a slot that repeats an earlier slot of its row is drawn again.  Stands in
 * for OpenGV's rand()-driven drawIndexSample.  OV2_EINVAL: n < 4, rows < 0, NULL out with rows > 0. */
int ov2_p3p_draw_samples(unsigned long long seed, int n, int rows, int *out);

/* ==================================================================== */
/* Per-frame pose (f15): MultiViewGeometry::ceresPnP in one launch      */
/* (src/multi_view_geometry.cpp:492-586) and VisualFrontEnd::computePose */
/* as one device-resident chain (src/visual_front_end.cpp:659-851)      */
/* ==================================================================== */
/* ov2_ceres_pnp[_batch]: the WHOLE two-pass protocol of ceresPnP in one kernel (csrc/pnp.hip, k_pnp_solve: one work-group per
 * problem, blockIdx.x = item; fp64), one upload, one launch, one download, one synchronisation per call:
 *   pass 1    Huber(sqrt(chi2th)) unless !use_robust, nmaxiter iterations, function_tolerance 1e-3, every other solver setting as
 *             ov2_ba_default_options gives it (Jacobi scaling, the LM diagonal bounds, radius 1e4 ...)
 *   outliers  block i is bad when chi2_i > chi2th or its depth is not positive, on the values of the LAST Evaluate of pass 1 (the
 *             candidate evaluation overwrites them whether or not the step is accepted), ascending
 *   all bad   (or n == 0) success = 0 with the pose of pass 1, no pass 2
 *   pass 2    only if apply_l2_after_robust and some block is bad: a fresh solve with the trivial loss over the remaining blocks,
 *             from the pose of pass 1
 *   success   Summary::IsSolutionUsable of the last solve that ran (termination OV2_TERM_NO_CONVERGENCE .. OV2_TERM_MIN_RADIUS)
 * The outlier list is that of the first test only.  The reference's max_solver_time_in_seconds = 0.005 has no counterpart: the
 * result never depends on machine load.  Every sum over the blocks (J^T J, J^T r, the cost) is formed in a fixed order, so a problem
 * gives the same bits from run to run, as item b of any batch, and inside ov2_compute_pose as here.  The trust-region rules are
 * those of ov2_ba_solve's pose-only kernel (csrc/ba_core.hpp); that kernel and the route through ov2_ba_solve are unchanged.
 *
 * ov2_compute_pose[_batch]: per item ONE upload, the three launches of ov2_p3p_ransac_batch, a gather launch, the k_pnp_solve launch,
 * a decision launch, ONE download, ONE synchronisation:
 *   1  n < 4: action OV2_POSE_TOO_FEW; Twc_out = Twc, p3p_req_out = p3p_req, nothing removed, nothing else ran (:667).
 *   2  do_p3p (the caller's bp3preq_ || dop3p_): the search of ov2_p3p_ransac_batch on bv / wpt / samples with params->p3p.  Status != 0,
 *      fewer than 5 inliers or a non-finite translation: action OV2_POSE_P3P_RESET, Twc_out = Twc, p3p_req_out = p3p_req (:750-761).
 *   3  otherwise P3P's outliers leave unpx / wpt / scale, the order of the rest kept (:769-778); P3P's pose (Rwc as the unit
 *      quaternion of ov2_pose_from_model) becomes the frame pose AND the start of PnP (:766).
 *   4  ceresPnP as above on the m remaining blocks.
 *   5  rejected when !success, or m - n_out < 5, or (double)n_out > 0.5 * (double)m, or the translation is not finite (:809-813):
 *        without P3P             OV2_POSE_PNP_REQ_P3P, p3p_req_out = 1, Twc_out = Twc
 *        with P3P and mono       OV2_POSE_PNP_RESET   } p3p_req_out = p3p_req, Twc_out = P3P's pose, P3P's removals stand,
 *        with P3P and stereo     OV2_POSE_PNP_KEEP    } PnP's do not
 *      accepted: OV2_POSE_OK, Twc_out = PnP's pose, p3p_req_out = 0, PnP's outliers are removed as well.
 *   removed[i], i in the caller's index space: 0 kept, 1 removed after P3P, 2 removed after an accepted PnP.
 * The chain gives, bit for bit, what ov2_p3p_ransac followed by ov2_ceres_pnp on the host-compacted arrays gives.
 *
 * Capacity: OV2_P3P_MAX_POINTS points and OV2_P3P_MAX_ROWS rows per item, 65535 items per call.  Items of a batch share params;
 * sizes may differ, empty items are allowed; the single forms are the batch forms with one item.  OV2_EINVAL: a NULL params /
 * problem / result / ctx, a NULL array with a non-zero count (bv and samples only where do_p3p), a negative count, a non-finite
 * input value, |scale| > 60, chi2th <= 0 or not finite, nmaxiter < 0, K not finite or fx / fy == 0, whatever ov2_p3p_ransac_batch
 * refuses in params->p3p, anything beyond the capacity.  All of it is checked on the host, the inputs before the context; a
 * rejected call leaves its outputs untouched. */
enum { OV2_POSE_TOO_FEW = 0, OV2_POSE_OK = 1, OV2_POSE_PNP_REQ_P3P = 2, OV2_POSE_P3P_RESET = 3, OV2_POSE_PNP_RESET = 4, OV2_POSE_PNP_KEEP = 5 };
typedef struct {
    int nmaxiter;                /* 5 in computePose                                                                         */
    double chi2th;               /* robust_mono_th (5.9915)                                                                  */
    int use_robust;              /* buse_robust                                                                              */
    int apply_l2_after_robust;   /* bapply_l2_after_robust                                                                   */
    double K[4];                 /* fx fy cx cy of the left camera                                                           */
} ov2_pnp_params;
typedef struct {
    int n;                       /* residual blocks                                                                          */
    const double *unpx;          /* 2 n: undistorted pixels                                                                  */
    const double *wpt;           /* 3 n: world points                                                                        */
    const int *scale;            /* n: pyramid level of the keypoint, sigma = 2^scale                                        */
    const double *Twc;           /* 7: [t q(xyzw)], the start                                                                */
} ov2_pnp_problem;
typedef struct {
    int ran;                     /* 0: the pass did not run (the other fields are 0 then)                                    */
    int iterations;              /* as ov2_ba_result                                                                         */
    int num_successful_steps;
    int termination;             /* OV2_TERM_*                                                                               */
    double initial_cost, final_cost;
} ov2_pnp_pass;
typedef struct {
    int success;
    int n_outliers;
    double Twc[7];
    int *outliers;               /* n slots; the first n_outliers are written, ascending                                     */
    ov2_pnp_pass pass[2];
} ov2_pnp_result;
int ov2_ceres_pnp(ov2_ctx *ctx, const ov2_pnp_params *params, const ov2_pnp_problem *problem, ov2_pnp_result *result);
int ov2_ceres_pnp_batch(ov2_ctx *ctx, const ov2_pnp_params *params, int n_items, const ov2_pnp_problem *problems,
                        ov2_pnp_result *results);

typedef struct {
    ov2_pnp_params pnp;
    ov2_p3p_params p3p;          /* the front end searches with OV2_P3P_LMEDS                                                */
    int mono;                    /* pslamstate_->mono_                                                                       */
} ov2_pose_params;
typedef struct {
    int n;                       /* 3-D keypoints of the frame (the packed arrays of :675-712)                               */
    const double *unpx;          /* 2 n                                                                                      */
    const double *wpt;           /* 3 n                                                                                      */
    const int *scale;            /* n                                                                                        */
    const double *Twc;           /* 7: the frame's pose                                                                      */
    const double *bv;            /* 3 n unit bearings; read only where do_p3p                                                */
    int do_p3p;                  /* bp3preq_ || dop3p_                                                                       */
    int p3p_req;                 /* bp3preq_                                                                                 */
    int n_rows;                  /* rows of the sample table; read only where do_p3p                                         */
    const int *samples;          /* 4 n_rows                                                                                 */
} ov2_pose_problem;
typedef struct {
    double Twc[7];
    int action;                  /* OV2_POSE_*                                                                               */
    int p3p_req_out;             /* the next frame's bp3preq_                                                                */
    int n_removed_p3p, n_outliers_pnp;   /* P3P's outliers (0 unless P3P succeeded); PnP's first-test outliers, accepted or not */
    int ran_p3p;                 /* the search ran for this item (do_p3p and n >= 4); pass[q].ran says the same of the PnP passes */
    int p3p_status, p3p_best_row, p3p_iterations, p3p_rows_consumed;   /* as ov2_p3p_result; 0 / -1 / 0 / 0 when it did not run */
    double p3p_score;
    uint8_t *removed;            /* n bytes                                                                                  */
    ov2_pnp_pass pass[2];
} ov2_pose_result;
int ov2_compute_pose(ov2_ctx *ctx, const ov2_pose_params *params, const ov2_pose_problem *problem, ov2_pose_result *result);
int ov2_compute_pose_batch(ov2_ctx *ctx, const ov2_pose_params *params, int n_items, const ov2_pose_problem *problems,
                           ov2_pose_result *results);
/* Host only: the pose [t q(xyzw)] of a P3P model (Rwc row-major, twc), with the very arithmetic the chain uses on the device
 * (Eigen's matrix-to-quaternion branches, then a normalisation), so that a caller who runs ov2_p3p_ransac and ov2_ceres_pnp
 * directly starts PnP from the same bits.  OV2_EINVAL: a NULL pointer. */
int ov2_pose_from_model(const double *model12, double *Twc7);

/* ==================================================================== */
/* Relative pose from 2D-2D matches (MultiViewGeometry::                */
/* compute5ptEssentialMatrix, src/multi_view_geometry.cpp:594-696,      */
/* USE_OPENGV)                                                          */
/* ==================================================================== */
/* What VisualFrontEnd::epipolar2d2dFiltering runs per frame, the initialisation once and the loop closer per candidate: Nister's
 * five-point solver on the first five matches of a sample row, all EIGHT matches of the row pick among its solutions (real roots
 * of the degree-10 polynomial x four decompositions), and the hypotheses are searched as OpenGV's sac::Ransac (largest inlier
 * count, adaptive iteration bound with a sample size of 8) would.  fp64 (csrc/fivept.hip): ONE staging upload, three launches, ONE
 * download, ONE synchronisation per call.
 *
 * The model is [R | t] with x1 = R x2 + t (the reference's Rwc, twc), |t| = 1: bv1^T [t]x R bv2 = 0.  The sample table is an
 * INPUT (n_rows x 8 indices), so the result is a deterministic function of the arguments.  A row with a repeated or out-of-range
 * index, without a real root or without a finite candidate is skipped WITHOUT counting an iteration.
 *   RANSAC  k = 1; while iterations < k: a strictly larger inlier count (d < threshold) becomes the best and sets
 *           k = log(1 - probability) / log(1 - (count / n)^8) (the argument clamped to [DBL_EPSILON, 1 - DBL_EPSILON]); ++iterations;
 *           stop once iterations > max_iterations.
 * d_i = (1 - bv1_i . p / |p|) + (1 - bv2_i . r / |r|), p the midpoint triangulation of the two rays (triangulate2), r = R^T (p - t).
 * After the loop the outliers of the best model are the points with d_i >= threshold (or d_i not a number), ascending.  The full
 * specification is tests/fivept_ref.py; OpenGV itself is not available to this project, so the solver and the loop are restated and
 * nothing is pinned against an OpenGV binary.
 *
 * status: OV2_EPI_TOO_FEW_POINTS (n < 8: nothing else is set or searched), OV2_EPI_NO_MODEL (no valid row was reached; comes with
 * OV2_EPI_FEW_INLIERS), OV2_EPI_FEW_INLIERS (fewer than 10, :665).  The reference returns false on any of them.
 *
 * boptimize must be 0: OpenGV's non-linear refinement (optimizeModelCoefficients on the inliers) is not provided.  The front end
 * asks for it only in the mono branch when tracking is poor (src/visual_front_end.cpp:440-660); every other caller passes false.
 *
 * Capacity: OV2_EPI_MAX_POINTS points and OV2_EPI_MAX_ROWS rows per problem, 65535 problems per call.  OV2_EINVAL: NULL params /
 * problem / result / ctx, a NULL array with a non-zero count, a negative count, a non-finite bearing, threshold <= 0 or not finite,
 * probability outside (0, 1), max_iterations < 0, boptimize != 0, anything beyond the capacity.  All of it is checked on the host
 * before any device work, the inputs before the context; a rejected call writes nothing. */
enum { OV2_EPI_TOO_FEW_POINTS = 1, OV2_EPI_NO_MODEL = 2, OV2_EPI_FEW_INLIERS = 4 };
#define OV2_EPI_MAX_POINTS 2048
#define OV2_EPI_MAX_ROWS 4096
typedef struct {
    int max_iterations;          /* nmaxiter                                                                                 */
    double threshold;            /* 2 (1 - cos(atan(errth / focal)))                                                         */
    double probability;          /* 0.99                                                                                     */
    int boptimize;               /* must be 0                                                                                */
} ov2_epipolar_params;
typedef struct {
    int n;                       /* matches                                                                                  */
    const double *bv1;           /* 3 n: unit bearing vectors of the keyframe                                                */
    const double *bv2;           /* 3 n: unit bearing vectors of the current frame                                           */
    int n_rows;                  /* rows of the sample table                                                                 */
    const int *samples;          /* 8 n_rows                                                                                 */
} ov2_epipolar_problem;
typedef struct {
    double model[12];            /* R row-major (9), t (3)                                                                   */
    double score;                /* the best row's inlier count                                                              */
    int best_row;                /* -1: no model                                                                             */
    int iterations;              /* rows that counted                                                                        */
    int rows_consumed;           /* rows the loop took from the table, skipped ones included                                 */
    int status;                  /* OV2_EPI_* bits, 0 = the reference returns true                                           */
    int n_inliers, n_outliers;
    int *outliers;               /* n slots; the first n_outliers are written, ascending                                     */
    uint8_t *trace_valid;        /* optional (NULL or n_rows): 1 where the row gave a hypothesis                             */
    double *trace_score;         /* optional (NULL or n_rows): every row's inlier count, 0 for an invalid row                */
    double *trace_model;         /* optional (NULL or 12 n_rows): every row's model, zeros for an invalid row                */
} ov2_epipolar_result;
/* one problem: the batch form with one item, through the same code path */
int ov2_epipolar_ransac(ov2_ctx *ctx, const ov2_epipolar_params *params, const ov2_epipolar_problem *problem,
                        ov2_epipolar_result *result);
/* the problems of a lock-step batch, items [0, n_items) with shared params (the problem is a grid axis: each kernel is launched
 * once).  Per item the result equals ov2_epipolar_ransac on that item bit for bit; sizes may differ, empty problems are allowed. */
int ov2_epipolar_ransac_batch(ov2_ctx *ctx, const ov2_epipolar_params *params, int n_items, const ov2_epipolar_problem *problems,
                              ov2_epipolar_result *results);
/* Host only: rows x 8 indices of [0, n), distinct inside a row, from the stream of ov2_p3p_draw_samples.  OV2_EINVAL: n < 8,
 * rows < 0, NULL out with rows > 0. */
int ov2_epipolar_draw_samples(unsigned long long seed, int n, int rows, int *out);

/* ==================================================================== */
/* Pose-graph optimisation (Optimizer::localPoseGraph,                  */
/* src/optimizer.cpp:2346-2591, and Optimizer::fullPoseGraph,           */
/* :2783-2865)                                                          */
/* ==================================================================== */
/* One ceres::Solve over SE(3) poses Twc ([tx ty tz qx qy qz qw], SE3LeftParameterization: T <- Exp(delta) T) tied by
 * LeftSE3RelativePoseError blocks (src/ceres_parametrization.cpp:30-102): for an edge (i, j) with measurement Tc_i c_j
 *   err = Twc_j^-1 Twc_i Tc_i c_j,   r = (1 / sigma) log(err)   (Sophus SE(3) log, [rho; omega]),
 * with the reference's approximate Jacobians as written there ("adapted from Strasdat"), not the derivative of r.
 * fp64 (csrc/posegraph.hip): ONE staging upload, ONE launch that runs the whole Levenberg-Marquardt loop (one work-group per
 * problem, the trust-region rules of the other device solvers), ONE download, ONE synchronisation per call.
 *
 * The two option sets of the reference, both SPARSE_NORMAL_CHOLESKY / LM without a loss function and Ceres' defaults elsewhere
 * (ov2_ba_default_options, then):
 *   localPoseGraph  max_iter 10,  function_tolerance 1e-4, huber_delta 0   (:2441-2446)
 *   fullPoseGraph   max_iter 100, function_tolerance 1e-6, huber_delta 0   (:2820-2825)
 * huber_delta > 0 is OV2_EUNSUPPORTED (the reference passes no loss function).  max_solver_time_s > 0 is OV2_EUNSUPPORTED too: the
 * loop runs inside one launch and, like ov2_structure_ba, has no clock to stop it (that solver ignores the field; this one
 * refuses it, so a caller does not believe in a limit that is not there).
 *
 * Structure.  Order the variable poses (pose_const[i] == 0) by their index.  An edge may join a variable pose and a constant
 * one, or two variable poses that are NEIGHBOURS in that order, in either direction and any number of times (with two poses the
 * chain edge and the loop edge of localPoseGraph are the same pair).  The normal matrix is then block-tridiagonal with 6x6
 * blocks and falls into independent segments wherever two neighbours share no edge; SPARSE_NORMAL_CHOLESKY's exact solve of
 * (J^T J + D^2) y = J^T r is a block Cholesky recurrence along each segment.  Both problems of the reference have this form.  An
 * edge between two variable poses that are not neighbours is OV2_EUNSUPPORTED (the message names the edge), i == j is
 * OV2_EINVAL; nothing is enqueued.
 *
 * Deviation from Ceres: an edge whose two ends are constant (two consecutive keyframes in fullPoseGraph) takes no part in the
 * program and none in initial_cost / final_cost.  Ceres would add it to both as "fixed cost", which nobody reads.  A variable
 * pose without an edge is not in the program either (as in Ceres) and comes back unchanged.
 *
 * A problem without a variable pose, or without an edge that touches one, returns OV2_OK with poses_out = poses, iterations = 0
 * and termination = OV2_TERM_FUNCTION_TOL (Ceres: "no non-constant parameter blocks").  A block factorisation that meets a
 * non-positive or non-finite pivot is an invalid step (the radius shrinks); a solve whose run of max_consecutive_invalid_steps
 * invalid steps ends on such a failure reports OV2_TERM_FAILURE and returns its INPUT poses (Ceres does not write back an unusable
 * solution).
 *
 * With OV2_OPT_BA_TRACE = 1, ov2_pose_graph_solve fills the context's iteration trace (ov2_ba_get_trace), with the meaning it has
 * for ov2_ba_solve.  A batch call records none, unless it has exactly one item.
 *
 * Capacity: OV2_PG_MAX_POSES poses and OV2_PG_MAX_EDGES edges per problem, 65535 problems per call.  OV2_EINVAL: a NULL
 * argument or array, a negative count, anything beyond the capacity, a pose / measurement / sigma that is not finite, a zero
 * quaternion, sigma <= 0, an edge index out of range, i == j, max_iter < 0.  Everything is checked on the host before the context
 * is looked at; a rejected call writes none of its outputs. */
#define OV2_PG_MAX_POSES 16384
#define OV2_PG_MAX_EDGES 32768
typedef struct {
    int n_poses;
    const double *poses;         /* 7 n_poses: Twc                                                                            */
    const uint8_t *pose_const;   /* n_poses: 1 = constant block (the loop keyframe; the keyframes of fullPoseGraph)           */
    int n_edges;
    const int *edge_i, *edge_j;  /* n_edges each                                                                              */
    const double *edge_T;        /* 7 n_edges: Tc_i c_j                                                                       */
    const double *edge_sigma;    /* n_edges, or NULL = 1 (both call sites of the reference)                                   */
} ov2_pg_problem;
typedef struct {
    double *poses_out;           /* 7 n_poses                                                                                 */
    int iterations, num_successful_steps;
    double initial_cost, final_cost;
    int termination;             /* OV2_TERM_*                                                                                */
    double solve_ms;             /* device time of the launch (the batch: of the whole batch)                                 */
} ov2_pg_result;
int ov2_pose_graph_solve(ov2_ctx *ctx, const ov2_pg_problem *p, const ov2_ba_options *o, ov2_pg_result *r);
/* n_items independent problems with shared options, one work-group each in the same launch.  Per item the result equals
 * ov2_pose_graph_solve on that item bit for bit; an item that fails (OV2_TERM_FAILURE) does not disturb the others. */
int ov2_pose_graph_solve_batch(ov2_ctx *ctx, int n_items, const ov2_pg_problem *p, const ov2_ba_options *o, ov2_pg_result *r);
/* What localPoseGraph does with the solution (:2476-2585), k_pg_apply.  win_old / win_new: the n_win window keyframes before and
 * after the solve.  Every younger keyframe and the current frame (young_old, n_young poses) get
 *   young_new = newopt_Twc (ini_Tcw young_old),
 * and every 3-D point moves rigidly with the keyframe it is anchored in (pt_kf in [0, n_win + n_young), the younger ones after
 * the window): xyz_out = Twc_new (Tcw_old xyz).  Quaternions are renormalised after each product, as Sophus::SE3d does.  The
 * 0.3 m test on the optimised pose of the new keyframe (:2467-2474, stereo only) is the caller's.  OV2_EINVAL: NULL array with a
 * non-zero count, negative count, n_win + n_young = 0 with n_pts > 0, pt_kf out of range, a pose that is not finite or has a
 * zero quaternion, more than 2^24 keyframes or 2^27 points. */
int ov2_pose_graph_apply(ov2_ctx *ctx, int n_win, const double *win_old, const double *win_new, const double ini_Tcw[7],
                         const double newopt_Twc[7], int n_young, const double *young_old, double *young_new, int n_pts,
                         const double *xyz, const int *pt_kf, double *xyz_out);

/* ---- frame versus previous keyframe (fkf.hip): the per-frame keypoint passes of src/visual_front_end.cpp -------------------
 *   ov2_parallax           VisualFrontEnd::computeParallax (:1066-1141) in the arithmetic of each of its three call sites
 *   ov2_kf_decision        VisualFrontEnd::checkNewKfReq (:986-1061): the rule on parallax, occupied cells and 3-D counts
 *   ov2_sampson_filter_2d  the Sampson pass over the 2-D keypoints after the 5-point search (:610-652)
 * One item describes the current frame and the previous keyframe from host arrays.  Frame::getKeypointById is a device-side
 * binary search of cur_lmid[i] in kf_lmid, which therefore has to be STRICTLY ASCENDING (the host does not join); landmark ids
 * are non-negative in the reference, and a current id that the keyframe does not hold has "no counterpart".
 * Poses are [tx ty tz qx qy qz qw] as the Frame holds them: kf_Tcw is the keyframe's own Tcw_, not re-derived from its Twc_.
 *
 * Parallax, for each current keypoint IN ARRAY ORDER (mapkps_ is an unordered_map: the caller's order is the only one there is):
 *   skipped by the filter (ONLY_2D: :1096; ONLY_3D: :494-498) or without counterpart (:1104 / :505): continue;
 *   unrot:  u = projectCamToImage(R bv) (camera_calibration.cpp:243-252), R = matrix(q of kf_Tcw) matrix(q of cur_Twc) (:1082-1084),
 *           both by Eigen's toRotationMatrix from the quaternions as held, sums of three products serial ((a0 + a1) + a2);
 *   else    u = cur_unpx[i];
 *   d = cv::norm(u - kf_unpx[j]): the difference in float, sqrt((double)dx dx + (double)dy dy);
 *   OV2_FKF_AVG / OV2_FKF_MEDIAN (:1117-1118): p = (float)d, sum += p in float;
 *   OV2_FKF_AVG_WIDE (:517): sum = (float)((double)sum + d) -- it differs from the former in the last bit.
 * The sum is serial in array order, not a tree.  Result: the averages are sum / (float)n, with n == 0 giving 0 (:1126) for AVG and
 * MEDIAN and the 0.f / 0 NaN of :528 for AVG_WIDE.  MEDIAN: the reference inserts into a std::set<float>, so it is the element
 * at index n_distinct / 2 of the DISTINCT values in ascending order, not the middle of the multiset.  n_distinct is 0 for the
 * averages (the set stays empty).  A non-finite p is undefined behaviour in the reference's set: here it is counted in
 * n_nonfinite, stays out of the distinct values, and with n_nonfinite > 0 the median is NaN; the averages carry the non-finite
 * value through the float sum like the reference.
 *
 * Decision: parallax with (unrot = 1, OV2_FKF_ALL, OV2_FKF_MEDIAN).  nb3dkps / noccupcells of the item, or with -1 counted here:
 * the cur_is3d flags set, and the distinct Frame::getKeypointCellIdx(cur_px) (frame.cpp:587-592: float division by ncellsize,
 * floor, r nbwcells + c).  An index outside [0, nbwcells nbhcells) would make the reference's vgridkps_.at() throw: it is not
 * counted and reported in n_out_of_grid (as is a row or column beyond +-2^20, or not finite).  The comparisons of :1005-1045 are
 * the reference's, in double against its size_t / int / float operands.  `reason`: the early return that fired (OV2_KF_RET_*),
 * or the bits of the final expression (c0 || c1 || c2) && cx.  With n_nonfinite > 0 the decision is 0 and reason
 * OV2_KF_NONFINITE.
 *
 * Sampson pass: for every current keypoint with is3d == 0, err = computeSampsonDistance(Fkfcur, cur_unpx, kf_unpx) with the
 * current point as leftpt, bad = err > fransac_err; 3-D keypoints get err = 0, bad = 0.  The reference does NOT check that the
 * keyframe holds the keypoint (:633): a missing counterpart is scored against Keypoint()'s unpx_ = (0, 0), and so it is here.
 * Fkfcur is the caller's (computeFundamentalMat12 in its own Eigen), row-major like the Frl of ov2_stereo_epipolar_check.
 *
 * Capacity: OV2_FKF_MAX_POINTS keypoints on either side, OV2_FKF_MAX_CELLS grid cells, 65535 items (OV2_EUNSUPPORTED beyond).
 * OV2_EINVAL: a NULL argument or array (cur_px / cur_bv / cur_Twc / kf_Tcw are not read by the Sampson pass and may be NULL
 * there), a negative count, kf_lmid not strictly ascending, ncellsize / nbwcells / nbhcells not positive (decision only).
 * All of it is checked on the host before the context is touched; a rejected call writes nothing.  Each call is one upload, one
 * launch, one download, one host synchronisation. */
#define OV2_FKF_MAX_POINTS 2048
#define OV2_FKF_MAX_CELLS 65536
enum { OV2_FKF_ALL = 0, OV2_FKF_ONLY_2D = 1, OV2_FKF_ONLY_3D = 2 };
enum { OV2_FKF_AVG = 0, OV2_FKF_MEDIAN = 1, OV2_FKF_AVG_WIDE = 2 };
enum {
    OV2_KF_C0 = 1, OV2_KF_C1 = 2, OV2_KF_C2 = 4, OV2_KF_CX = 8,     /* the final expression, :1036-1045                      */
    OV2_KF_RET_FEW_CELLS = 16,                                      /* :1008, true                                           */
    OV2_KF_RET_FEW_3D = 32,                                         /* :1015, true                                           */
    OV2_KF_RET_MANY_3D = 64,                                        /* :1021, false                                          */
    OV2_KF_RET_TIME = 128,                                          /* :1030, true                                           */
    OV2_KF_NONFINITE = 256,
    OV2_KF_FIRST_FRAME = 512,                                       /* ov2_btracker_track_mono: trackMono :77, true          */
    OV2_KF_NO_KEYFRAME = 1024                                       /* ov2_btracker_track_mono: no keyframe (info), :994     */
};
typedef struct {
    double K[4];                 /* fx fy cx cy of the left camera                                                           */
    int ncellsize, nbwcells, nbhcells;   /* the Frame's grid (frame.cpp:66-69)                                               */
    int nbmaxkps;                /* SlamParams::nbmaxkps_                                                                    */
    float finit_parallax;        /* SlamParams::finit_parallax_                                                              */
    int stereo;                  /* SlamParams::stereo_                                                                      */
} ov2_fkf_params;
typedef struct {
    int n_cur;
    const int *cur_lmid;         /* n_cur                                                                                    */
    const float *cur_px;         /* 2 n_cur: Keypoint::px_                                                                   */
    const float *cur_unpx;       /* 2 n_cur: Keypoint::unpx_                                                                 */
    const double *cur_bv;        /* 3 n_cur: Keypoint::bv_                                                                   */
    const uint8_t *cur_is3d;     /* n_cur                                                                                    */
    const double *cur_Twc;       /* 7                                                                                        */
    int n_kf;
    const int *kf_lmid;          /* n_kf, strictly ascending                                                                 */
    const float *kf_unpx;        /* 2 n_kf                                                                                   */
    const double *kf_Tcw;        /* 7                                                                                        */
    int cur_id, kf_id;           /* Frame::id_                                                                               */
    double cur_time, kf_time;    /* Frame::img_time_                                                                         */
    int kf_nb3dkps;              /* pkf->nb3dkps_                                                                            */
    int localba_is_on;           /* SlamParams::blocalba_is_on_                                                              */
    int noccupcells, nb3dkps;    /* of the current frame; -1: counted on the device from cur_px / cur_is3d                   */
} ov2_fkf_item;
typedef struct {
    float parallax;
    int n;                       /* keypoints that entered the statistic                                                     */
    int n_distinct;              /* size of the reference's set (MEDIAN), 0 otherwise                                        */
    int n_nonfinite;
} ov2_parallax_result;
typedef struct {
    float parallax;
    int n, n_distinct, n_nonfinite;
    int noccupcells, nb3dkps;    /* as used by the rule: the item's, or counted                                              */
    int n_out_of_grid;           /* 0 unless noccupcells was counted                                                         */
    int decision;                /* 0 / 1: checkNewKfReq's return value                                                      */
    int reason;                  /* OV2_KF_* bits                                                                            */
} ov2_kf_decision_result;
typedef struct {
    float *err;                  /* n_cur                                                                                    */
    uint8_t *bad;                /* n_cur                                                                                    */
    int n_bad;
} ov2_sampson2d_result;
int ov2_parallax(ov2_ctx *ctx, const ov2_fkf_params *params, const ov2_fkf_item *item, int unrot, int filter, int stat,
                 ov2_parallax_result *result);
int ov2_parallax_batch(ov2_ctx *ctx, const ov2_fkf_params *params, int n_items, const ov2_fkf_item *items, int unrot, int filter,
                       int stat, ov2_parallax_result *results);
int ov2_kf_decision(ov2_ctx *ctx, const ov2_fkf_params *params, const ov2_fkf_item *item, ov2_kf_decision_result *result);
int ov2_kf_decision_batch(ov2_ctx *ctx, const ov2_fkf_params *params, int n_items, const ov2_fkf_item *items,
                          ov2_kf_decision_result *results);
/* one Fkfcur (9 doubles, row-major) per item */
int ov2_sampson_filter_2d(ov2_ctx *ctx, const ov2_fkf_item *item, const double Fkfcur[9], float fransac_err,
                          ov2_sampson2d_result *result);
int ov2_sampson_filter_2d_batch(ov2_ctx *ctx, int n_items, const ov2_fkf_item *items, const double *Fkfcur, float fransac_err,
                                ov2_sampson2d_result *results);

/* ---- epipolar2d2dFiltering (epifilter.hip): VisualFrontEnd::epipolar2d2dFiltering, src/visual_front_end.cpp:440-656 -----------
 * The whole per-frame function as ONE device chain: the join against the previous keyframe, the parallax gate, the 5-point search
 * over a sample table drawn on the device, the 50 % rule, the removals, the mono pose, computeFundamentalMat12 and the Sampson pass
 * over the 2-D keypoints.  One upload, five launches (k_epif_gather, k_e5_solve, k_e5_score, k_e5_pick, k_epif_decide), one
 * download, ONE synchronisation per call.  The arithmetic is that of the three separate calls: the parallax IS ov2_parallax(unrot =
 * 1, ONLY_3D or ALL, OV2_FKF_AVG_WIDE), the search IS ov2_epipolar_ransac on the packed bearings with the table of
 * ov2_epipolar_draw_samples(seed, m, n_rows), the pass IS ov2_sampson_filter_2d -- bit for bit.
 *
 *   :462   n_cur < 8: OV2_EPIF_TOO_FEW_KPS.  (m, parallax, epifrom3dkps and nb3dkps are still reported; nothing is searched.)
 *   :484   epifrom3dkps = stereo && nb3dkps > 30; nb3dkps is the item's, or with -1 the cur_is3d flags set.
 *   :492   the join: the current keypoints IN ARRAY ORDER, only the 3-D ones under epifrom3dkps; the counterpart by binary search in
 *          the strictly ascending kf_lmid, a keypoint without one is skipped.  Match k (k < m) is current keypoint pair_cur[k] and
 *          keyframe slot j: bv1[k] = kf_bv[j], bv2[k] = cur_bv[pair_cur[k]].
 *   :528   parallax = sum / (float)m, the sum serial in array order as OV2_FKF_AVG_WIDE; m == 0 gives the reference's 0.f / 0 NaN.
 *   :530   (double)parallax < 2. * (double)fransac_err: OV2_EPIF_LOW_PARALLAX.  A NaN parallax does not return here.
 *   :540   do_optimize = mono && nbkfs > 2 && nb3dkps < 30.
 *   :559   the search (epi.max_iterations / threshold / probability), over n_rows rows when m >= 8 and without a table otherwise.
 *   :574   any OV2_EPI_* bit in its status (m < 8 included): OV2_EPIF_NO_MODEL.
 *   :580   (double)n_outliers > 0.5 * (double)m: OV2_EPIF_DEGENERATE, nothing is removed.
 *   :587   removed[pair_cur[outliers[k]]] = 1.
 *   :594   do_optimize: see "Mono" below.
 *   :611   epifrom3dkps: F = K^-T hat(t) R' K^-1 with t = model t, R' = toRotationMatrix of the quaternion of model R (the reference
 *          goes through Sophus::SE3d(Rkfc, tkfc) and back: Eigen's matrix-to-quaternion branches, a normalisation), K^-1 and K^-T
 *          in closed form for the upper-triangular K ([1/fx 0 -cx/fx; 0 1/fy -cy/fy; 0 0 1]), the products from left to right as
 *          full 3 x 3 products, each sum of three terms serial.  Then for every keypoint with is3d == 0 the rule of
 *          ov2_sampson_filter_2d (the current point as leftpt, a missing counterpart scored against (0, 0)):
 *          err > fransac_err gives removed = 2.  F is restated, not pinned against an Eigen / Sophus build.
 *          OV2_EPIF_FILTERED.
 *
 * Mono.  boptimize changes only Rwc / twc in the reference's search, never its outlier list (src/multi_view_geometry.cpp:669-693),
 * so every decision and every removal above is the reference's in this branch too.  The REFINED pose is not available (OpenGV's
 * non-linear refinement has no device form; epi.boptimize must be 0).  Where do_optimize holds and the filter reached :594 the
 * chain sets pose_from_model = 1 and writes
 *   Twc_model = kf_Twc * SE3(Rkfc, scale * tkfc / |tkfc|),   scale = |(kf_Tcw * cur_Twc).translation()|,
 * from the UNREFINED model in Sophus' arithmetic (SE3(R, t): the quaternion of ov2_pose_from_model; the product: quaternion product
 * with renormalisation plus the rotated translation, as ov2_pose_graph_apply).  This is NOT the reference's pose until a
 * refinement exists: the chain never overwrites the caller's pose, and what to do with Twc_model is the caller's decision.
 *
 * Device draw.  The table is drawn by k_epif_gather because m exists only on the device in a fused step; it equals
 * ov2_epipolar_draw_samples(seed, m, n_rows) integer for integer.  The kernel evaluates the stream in windows of 2048 draws; a row
 * that needed more than a WHOLE window by itself (2048 draws: a chance below 2^-380 at m = 8, where a row is a permutation and
 * misses a given value for 2048 draws with probability (7/8)^2048) ends the draw, and the remaining rows are filled with
 * -1, which the search skips.
 *
 * Capacity: OV2_FKF_MAX_POINTS keypoints on either side, OV2_EPI_MAX_ROWS rows, 65535 items.  OV2_EINVAL, all of it checked on the
 * host before the context is touched (a rejected call writes nothing): everything ov2_parallax and ov2_epipolar_ransac_batch refuse
 * for these inputs (NULL arguments or arrays with a non-zero count, negative counts, kf_lmid not strictly ascending, threshold,
 * probability, max_iterations, boptimize != 0), a NULL kf_bv / kf_Twc with n_kf > 0, a NULL `removed` with n_cur > 0, bearings,
 * poses or K that are not finite, n_rows outside [0, OV2_EPI_MAX_ROWS], n_cur / n_kf beyond OV2_FKF_MAX_POINTS, more than 65535
 * items. */
enum { OV2_EPIF_TOO_FEW_KPS = 0, OV2_EPIF_LOW_PARALLAX = 1, OV2_EPIF_NO_MODEL = 2, OV2_EPIF_DEGENERATE = 3, OV2_EPIF_FILTERED = 4 };
typedef struct {
    ov2_fkf_params fkf;          /* K and stereo are read                                                                    */
    ov2_epipolar_params epi;     /* nransac_iter_, the bearing threshold of fransac_err_, 0.99; boptimize must be 0          */
    float fransac_err;           /* SlamParams::fransac_err_ (pixels): the gate and the Sampson pass                         */
    int mono;                    /* SlamParams::mono_                                                                        */
    int n_rows;                  /* rows of the sample table drawn per item that searches                                    */
} ov2_epifilter_params;
typedef struct {
    ov2_fkf_item fkf;            /* the item of ov2_parallax / ov2_sampson_filter_2d; nb3dkps: pcurframe_->nb3dkps_ or -1    */
    const double *kf_bv;         /* 3 n_kf: the keyframe's Keypoint::bv_, in the order of kf_lmid                            */
    const double *kf_Twc;        /* 7: pkf->getTwc() as held                                                                 */
    int nbkfs;                   /* pmap_->nbkfs_                                                                            */
    unsigned long long seed;     /* of the sample table                                                                      */
} ov2_epifilter_item;
typedef struct {
    int action;                  /* OV2_EPIF_*                                                                               */
    int m;                       /* matches that entered the search                                                          */
    int epifrom3dkps, do_optimize;
    int nb3dkps;                 /* as used: the item's, or counted                                                          */
    float parallax;              /* :528; NaN when m == 0                                                                    */
    int status, best_row, iterations, rows_consumed;   /* the search's, as ov2_epipolar_result; 0 / -1 / 0 / 0 when it did not run */
    double score;
    int n_inliers, n_outliers;
    double model[12];            /* Rkfc row-major, tkfc; zeros without a model                                              */
    double F[9];                 /* row-major; zeros unless the Sampson pass ran                                             */
    int n_removed_ransac, n_removed_sampson;
    uint8_t *removed;            /* n_cur bytes: 0 kept, 1 removed as a RANSAC outlier, 2 removed by the Sampson pass        */
    int *pair_cur;               /* optional (NULL or n_cur ints of room): the current index of packed match k, k < m        */
    float *err;                  /* optional (NULL or n_cur): the Sampson error, 0 where the pass did not score              */
    int pose_from_model;         /* 1: Twc_model is set (mono, see above)                                                    */
    double Twc_model[7];
    int *trace_samples;          /* optional diagnostic (NULL or 8 n_rows): the table the device drew; untouched without a search */
} ov2_epifilter_result;
/* The four pointers of the result (removed, pair_cur, err, trace_samples) are INPUTS of the call, read on entry: the caller sets
 * each of them to a buffer or to NULL before the call (zero-initialise the struct, then set `removed`); every other field is
 * written by the call.  trace_samples is not part of the reference's function: it exists so that the table drawn on the device can
 * be compared with ov2_epipolar_draw_samples. */
/* one frame: the batch form with one item, through the same code path */
int ov2_epipolar_filter(ov2_ctx *ctx, const ov2_epifilter_params *params, const ov2_epifilter_item *item, ov2_epifilter_result *result);
/* the frames of a lock-step batch with shared params (the item is a grid axis: each kernel is launched once).  Per item the result
 * equals ov2_epipolar_filter on that item bit for bit; sizes may differ, empty frames are allowed. */
int ov2_epipolar_filter_batch(ov2_ctx *ctx, const ov2_epifilter_params *params, int n_items, const ov2_epifilter_item *items,
                              ov2_epifilter_result *results);

/* ---- mono initialisation (monoinit.hip): trackMono's un-initialised branch, src/visual_front_end.cpp:98-113, with
 * VisualFrontEnd::checkReadyForInit, :855-984 -------------------------------------------------------------------------------------
 * The whole decision "can this mono system initialise from the previous keyframe and this frame" as ONE device chain: the count of
 * 2-D keypoints, the plain median parallax, the join against the keyframe, the rotation-compensated average parallax in the
 * arithmetic of :908-913, the 5-point search over a sample table drawn on the device, the removals and the initial pose.  One upload,
 * six launches (k_fkf_parallax, k_minit_gather, k_e5_solve, k_e5_score, k_e5_pick, k_minit_decide), one download, ONE synchronisation
 * per call.  The frame's keypoints are taken in array order (the iteration order of pcurframe_->mapkps_, as ov2_epipolar_filter).
 *
 *   :100   nb2dkps = #(cur_is3d == 0); nb2dkps < min_2d_kps: OV2_MINIT_RESET (breset_req_).  Nothing else runs: every other field
 *          of the record is 0 (best_row -1), nothing is removed.  min_2d_kps is the reference's literal 50; 0 disables the test.
 *   :857   p0 IS ov2_parallax(unrot = 0, OV2_FKF_ALL, OV2_FKF_MEDIAN) bit for bit -- the median of the DISTINCT float parallaxes,
 *          0 when nothing joins, NaN when one of them is not finite -- reported with its n / n_distinct / n_nonfinite.
 *   :861   the gate is (double)p0 > (double)finit_parallax (strict: equality does not pass, nor does NaN); failing it:
 *          OV2_MINIT_LOW_PARALLAX.
 *   :873   n_cur < 8: OV2_MINIT_TOO_FEW_KPS.
 *   :887   Rkfcur = toRotationMatrix(kf_Tcw.q) * toRotationMatrix(cur_Twc.q), as ov2_parallax(unrot = 1).
 *   :893   the join of ov2_epipolar_filter without its 3-D restriction: EVERY current keypoint in array order, its counterpart by
 *          binary search in the strictly ascending kf_lmid, a keypoint without one is skipped.  Match k (k < m) is current keypoint
 *          pair_cur[k] and keyframe slot j: bv1[k] = kf_bv[j], bv2[k] = cur_bv[pair_cur[k]].
 *   :908   the parallax of a match is NOT the distance of ov2_parallax(unrot = 1) (projectCamToImage multiplies by 1 / z and adds
 *          the principal point; this line multiplies by the matrix K and divides):
 *            rotbv = Rkfcur bv, each coefficient the serial sum (r0 x + r1 y) + r2 z;
 *            u = K rotbv with K = [fx 0 cx; 0 fy cy; 0 0 1] as a full 3 x 3 by 3 coefficient product, zero entries included:
 *                u.x = (fx x + 0 y) + cx z,  u.y = (0 x + fy y) + cy z,  u.z = (0 x + 0 y) + 1 z;
 *            rotpx = ((float)(u.x / u.z), (float)(u.y / u.z));
 *            d = cv::norm(rotpx - kf_unpx): the difference in float, then sqrt((double)dx dx + (double)dy dy).
 *          The sum is OV2_FKF_AVG_WIDE's: sum = (float)((double)sum + d), serial in array order.  This form is restated from the
 *          reference's source, not pinned against an Eigen build.
 *   :917   m < 8: OV2_MINIT_TOO_FEW_MATCHES (p1 is reported as 0: the reference returns before it divides).
 *   :923   p1 = sum / (float)m;  p1 < finit_parallax (float against float, strict: equality passes, and so does NaN):
 *          OV2_MINIT_LOW_ROT_PARALLAX.
 *   :945   the search IS ov2_epipolar_ransac on the packed bearings with the table of ov2_epipolar_draw_samples(seed, m, n_rows),
 *          drawn on the device as in ov2_epipolar_filter.  Any OV2_EPI_* bit in its status (fewer than 10 inliers included):
 *          OV2_MINIT_NO_MODEL, nothing is removed.
 *   :962   removed[pair_cur[outliers[k]]] = 1 for every outlier.  There is no 50 % rule here.
 *   :968   t = tkfc / |tkfc| (the norm as sqrt((x x + y y) + z z), a division per component, as Twc_model of ov2_epipolar_filter),
 *          then t * 0.25 per component.  Twc_init = [t, q], q the quaternion of ov2_pose_from_model(model) (Frame::setTwc(R, t):
 *          setRotationMatrix, then the translation).  OV2_MINIT_READY.
 *
 * The one deviation.  The reference calls the search with do_optimize = true.  That changes only Rwc / twc, never the outlier list
 * (src/multi_view_geometry.cpp:669-693), so every action and every removal above is the reference's.  The REFINED model is not
 * available (OpenGV's non-linear refinement has no device form; epi.boptimize must be 0): Twc_init comes from the UNREFINED model and
 * the record says so with pose_refined = 0.  This is NOT the reference's pose until a refinement exists.
 *
 * A field that a return above comes before is 0 (best_row -1): p0 and its counts are set unless the action is OV2_MINIT_RESET; m
 * from :917 on; p1 from :923 on; the search's fields where it ran; model / Twc_init / n_removed with OV2_MINIT_READY (model also
 * with OV2_MINIT_NO_MODEL, as the search left it).  `removed` is always written (n_cur bytes).
 *
 * Capacity: OV2_FKF_MAX_POINTS keypoints on either side, OV2_EPI_MAX_ROWS rows, 65535 items.  OV2_EINVAL, all of it checked on the
 * host before the context is touched (a rejected call writes nothing): everything ov2_epipolar_filter_batch refuses for the same
 * fields (NULL arguments or arrays with a non-zero count -- cur_px included, the item is ov2_parallax's --, negative counts, kf_lmid
 * not strictly ascending, threshold, probability, max_iterations, boptimize != 0, a NULL kf_bv with n_kf > 0, a NULL `removed` with
 * n_cur > 0, bearings, poses or K that are not finite, n_rows outside [0, OV2_EPI_MAX_ROWS], n_cur / n_kf beyond OV2_FKF_MAX_POINTS,
 * more than 65535 items), min_2d_kps < 0, a finit_parallax that is not finite. */
enum {
    OV2_MINIT_RESET = 0, OV2_MINIT_LOW_PARALLAX = 1, OV2_MINIT_TOO_FEW_KPS = 2, OV2_MINIT_TOO_FEW_MATCHES = 3,
    OV2_MINIT_LOW_ROT_PARALLAX = 4, OV2_MINIT_NO_MODEL = 5, OV2_MINIT_READY = 6,
    OV2_MINIT_NOT_REQUESTED = 7, OV2_MINIT_NO_KEYFRAME = 8       /* ov2_btracker_mono_init only */
};
typedef struct {
    ov2_fkf_params fkf;          /* K and finit_parallax are read                                                            */
    ov2_epipolar_params epi;     /* nransac_iter_, the bearing threshold of fransac_err_, 0.99; boptimize must be 0          */
    int n_rows;                  /* rows of the sample table drawn per item that searches                                    */
    int min_2d_kps;              /* :100, the reference's literal 50; 0: no such test                                        */
} ov2_mono_init_params;
typedef struct {
    ov2_fkf_item fkf;            /* the item of ov2_parallax                                                                 */
    const double *kf_bv;         /* 3 n_kf: the keyframe's Keypoint::bv_, in the order of kf_lmid                            */
    unsigned long long seed;     /* of the sample table                                                                      */
} ov2_mono_init_item;
typedef struct {
    int action;                  /* OV2_MINIT_*                                                                              */
    int nb2dkps;                 /* :100                                                                                     */
    float p0;                    /* :857                                                                                     */
    int p0_n, p0_n_distinct, p0_n_nonfinite;   /* as ov2_parallax_result                                                     */
    int m;                       /* matches that entered the search                                                          */
    float p1;                    /* :923                                                                                     */
    int status, best_row, iterations, rows_consumed;   /* the search's, as ov2_epipolar_result; 0 / -1 / 0 / 0 when it did not run */
    double score;
    int n_inliers, n_outliers;
    double model[12];            /* Rkfc row-major, tkfc; zeros without a model                                              */
    int n_removed;
    int pose_refined;            /* always 0: Twc_init is the pose of the UNREFINED model (see above)                        */
    double Twc_init[7];          /* OV2_MINIT_READY: [0.25 tkfc / |tkfc|, q(Rkfc)]; zeros otherwise                          */
    uint8_t *removed;            /* n_cur bytes: 0 kept, 1 removed as a RANSAC outlier                                       */
    int *pair_cur;               /* optional (NULL or n_cur ints of room): the current index of packed match k, k < m        */
    int *trace_samples;          /* optional diagnostic (NULL or 8 n_rows): the table the device drew; untouched without a search */
} ov2_mono_init_result;
/* The three pointers of the result are INPUTS of the call, read on entry, as those of ov2_epifilter_result. */
/* one frame: the batch form with one item, through the same code path */
int ov2_mono_init(ov2_ctx *ctx, const ov2_mono_init_params *params, const ov2_mono_init_item *item, ov2_mono_init_result *result);
/* the frames of a lock-step batch with shared params (the item is a grid axis: each kernel is launched once).  Per item the result
 * equals ov2_mono_init on that item bit for bit; sizes may differ, empty frames and empty keyframes are allowed. */
int ov2_mono_init_batch(ov2_ctx *ctx, const ov2_mono_init_params *params, int n_items, const ov2_mono_init_item *items,
                        ov2_mono_init_result *results);

/* ---- tracking priors (priors.hip): where the reference derives the priors that its KLT calls start from ----------------------
 *   ov2_klt_priors      VisualFrontEnd::kltTracking (src/visual_front_end.cpp:156-184): the map point of every 3-D keypoint
 *                       projected with the predicted pose (Frame::projWorldToImageDist, Frame::isInImage)
 *   ov2_stereo_priors   MapManager::stereoMatching (src/map_manager.cpp:396-489): the map point projected into the right image
 *                       (projWorldToRightImageDist, isInRightImage) and, without rectification (:438-484), the inverse-distance-
 *                       weighted depth of the 3-D neighbours of Frame::getSurroundingKeypoints(const Keypoint&) (frame.cpp:594-622)
 *                       pushed through projCamToRightImageDist
 * One lane per keypoint, fp64 without contraction; poses are [tx ty tz qx qy qz qw] as held.  The caller passes the predicted
 * pose: MotionModel is not part of this.
 *
 * Frame form, per keypoint:
 *   campt  = Tcw * wpt                          (Sophus SE3d * Vector3d; Tcw = the predicted Twc, inverted by the caller)
 *   projpx = projectCamToImageDist(campt)       (camera_calibration.cpp:254-281, as ov2_match_to_map)
 *   has_prior = klt_use_prior && is3d && projpx in [0, img_w) x [0, img_h);  prior = has_prior ? projpx : px
 * THERE IS NO DEPTH GATE, as there is none in the reference: a point behind the camera may project into the image and then
 * carries a prior.  NaN / infinity fails isInImage.  wpt is not read where is3d == 0.
 *
 * Stereo form, per keypoint, by `state` (0 = 2-D; 1 = 3-D with a live map point; 2 = 3-D whose map point is gone: the reference
 * removes the observation and `continue`s, :415-418):
 *   state 2   has_prior = 0, skip = 1
 *   state 1   projpt = rightcam.projectCamToImageDist(Tcic0 * (Tcw * wpt)); in the right image: has_prior = 1, done;
 *             else it falls through to the neighbour branch, as in the reference
 *   rect != 0 stop: the SAD prior lives inside ov2_stereo_match
 *   neighbours  rkp / ckp = floor(px.y / ncellsize) / floor(px.x / ncellsize) (float division); cells (rkp-1, ckp-1),
 *             (rkp-1, ckp), (rkp, ckp-1), (rkp, ckp) in that order, r < 0 / c < 0 skipped, cell_kp order inside a cell; the
 *             keypoint itself excluded; neighbours with state == 1 kept.  Per kept neighbour, in that order, double accumulators:
 *                coef = 1. / cv::norm(cokp.unpx - kp.unpx)   (difference in float, norm in double)
 *                weights += coef;  mean_z += coef * (Tcw * wpt_co).z
 *             With at least one: mean_z /= weights; pred = mean_z * (bv / bv.z) (component-wise division first);
 *             projpt = rightcam.projectCamToImageDist(Tcic0 * pred); in the right image: has_prior = 2.
 *             A coincident neighbour gives coef = inf, hence NaN, hence no prior, as in the reference.
 *   A row or column of the 2 x 2 block that lies outside the grid (px outside the image, or not finite) is skipped where the
 *   reference's vgridkps_.at() would throw or wrap.  The grid is ceil(img_w / ncellsize) x ceil(img_h / ncellsize) in float
 *   (frame.cpp:41-43): the two cameras of a rig share one image size.
 * Outputs: prior (px where there is none), has_prior (0 / 1 / 2), skip.  prior and has_prior ARE EXACTLY what
 * ov2_stereo_match[_batch] takes as priors3d_h and has_prior3d_h: non-zero means a prior (both kinds join v3dpriors, :411 / :477).
 *
 * OV2_EINVAL: a NULL argument, a negative count, a NULL array with a non-zero count, cell_kp outside its table, cell_start that
 * does not start at 0 or decreases, img_w / img_h / ncellsize not positive, state > 2.  OV2_EUNSUPPORTED: a coefficient count the
 * model does not take (pinhole 0 / 4 / 5 / 8 / 12, fisheye 0 / 4), more than 65535 items, more than 2^31 - 1 elements of one kind.
 * All of it is checked on the host before the context is touched; a rejected call writes nothing.  An item without keypoints is
 * allowed.  Each call is one upload, one launch, one download, one host synchronisation. */
typedef struct {
    int model;                   /* OV2_CAM_PINHOLE / OV2_CAM_FISHEYE: the left camera                                       */
    double K[4];                 /* fx fy cx cy                                                                              */
    const double *D;             /* nD distortion coefficients (NULL when nD == 0)                                           */
    int nD;
    double img_w, img_h;         /* pcalib_leftcam_->img_w_ / img_h_                                                         */
    int klt_use_prior;           /* SlamParams::klt_use_prior_                                                               */
} ov2_klt_priors_params;
typedef struct {
    const double *Tcw;           /* 7: the predicted pose, already inverted                                                  */
    int n;
    const float *px;             /* 2 n: Keypoint::px_                                                                       */
    const uint8_t *is3d;         /* n                                                                                        */
    const double *wpt;           /* 3 n: the map point (not read where is3d == 0)                                            */
} ov2_klt_priors_item;
typedef struct {
    float *prior;                /* 2 n                                                                                      */
    uint8_t *has_prior;          /* n: 0 / 1                                                                                 */
    int n_prior;                 /* keypoints with a prior                                                                   */
} ov2_klt_priors_result;
typedef struct {
    int model;                   /* the RIGHT camera                                                                         */
    double K[4];
    const double *D;
    int nD;
    double img_w, img_h;         /* pcalib_rightcam_->img_w_ / img_h_; also the size behind the keypoint grid                */
    double Tcic0[7];             /* pcalib_rightcam_->Tcic0_                                                                 */
    int ncellsize;               /* Frame::ncellsize_                                                                        */
    int rect;                    /* SlamParams::bdo_stereo_rect_                                                             */
} ov2_stereo_priors_params;
typedef struct {
    const double *Tcw;           /* 7: the keyframe's Tcw_                                                                   */
    int n;
    const float *px;             /* 2 n: px_                                                                                 */
    const float *unpx;           /* 2 n: unpx_                                                                               */
    const double *bv;            /* 3 n: bv_                                                                                 */
    const double *wpt;           /* 3 n: the map point (read where state == 1)                                               */
    const uint8_t *state;        /* n: 0 / 1 / 2                                                                             */
    const int *cell_start;       /* ncells + 1 offsets into cell_kp, as in ov2_match_keyframe (may be NULL when rect != 0)   */
    const int *cell_kp;          /* keypoint rows, per cell in vgridkps_ order                                               */
} ov2_stereo_priors_item;
typedef struct {
    float *prior;                /* 2 n: priors3d_h of ov2_stereo_match                                                      */
    uint8_t *has_prior;          /* n: 0, 1 (map point) or 2 (neighbours): has_prior3d_h of ov2_stereo_match                 */
    uint8_t *skip;               /* n: 1 = the reference drops the keypoint from the matching (state 2)                      */
    int n_prior3d, n_prior_nb, n_skip;
} ov2_stereo_priors_result;
/* one frame / keyframe: the batch form with one item, through the same code path */
int ov2_klt_priors(ov2_ctx *ctx, const ov2_klt_priors_params *params, const ov2_klt_priors_item *item, ov2_klt_priors_result *result);
int ov2_klt_priors_batch(ov2_ctx *ctx, const ov2_klt_priors_params *params, int n_items, const ov2_klt_priors_item *items,
                         ov2_klt_priors_result *results);
int ov2_stereo_priors(ov2_ctx *ctx, const ov2_stereo_priors_params *params, const ov2_stereo_priors_item *item,
                      ov2_stereo_priors_result *result);
int ov2_stereo_priors_batch(ov2_ctx *ctx, const ov2_stereo_priors_params *params, int n_items, const ov2_stereo_priors_item *items,
                            ov2_stereo_priors_result *results);

/* The lock-step step with the frame form fused in: ov2_btracker_track_frame[_begin] with prior_xy_h / has_prior_h replaced by
 * the map points (wpt_h: 3 doubles per slot, is3d_h: one byte per slot, both n_max slots per item) and the predicted poses
 * (Tcw_h: 7 doubles per item).  k_prior_frame writes the prior and flag slots of the tracker's point block on the context's
 * stream ahead of the tracking kernels: the priors never visit the host on the way in.  They come back with the results, so
 * the p3p rule runs on the flags the device set; ov2_btracker_track_frame_end finishes either kind of step, and
 * ov2_btracker_last_priors returns what was used.  The camera is the one of ov2_btracker_set_calibration (OV2_EINVAL without
 * one; the image size is the tracker's).  First frame, n_total == 0, the look-ahead calls and every result are as for
 * ov2_btracker_track_frame fed the output of ov2_klt_priors_batch (tests/test_gpu_priors_lockstep.py). */
int  ov2_btracker_track_frame_map_begin(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride, const float *kps_xy_h,
                                        const double *wpt_h, const uint8_t *is3d_h, const double *Tcw_h, const int *n_h,
                                        int klt_use_prior);
int  ov2_btracker_track_frame_map(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride, const float *kps_xy_h,
                                  const double *wpt_h, const uint8_t *is3d_h, const double *Tcw_h, const int *n_h, int klt_use_prior,
                                  float *out_xy_h, uint8_t *status_h, int *p3p_req);
/* prior (2 floats) / has_prior of the first n keypoints of item `item` as the LAST step used them (either form) */
int  ov2_btracker_last_priors(const ov2_btracker *t, int item, int n, float *prior_xy_h, uint8_t *has_prior_h);

/* The lock-step step with the per-frame pose fused in (f16): ov2_btracker_track_frame_map[_begin] followed, on the same stream and
 * with no host round trip in between, by ov2_compute_pose's chain on the frame's 3-D keypoints (VisualFrontEnd::trackMono,
 * src/visual_front_end.cpp:86-116 with doepipolar_ == 0, then computePose, :659-851).  One enqueue, one synchronisation (in _end).
 * Per active item b:
 *   tracking   exactly ov2_btracker_track_frame_map: Tcw_h is the predicted pose INVERTED by the caller, input->Twc_h the same pose
 *              NOT inverted (pcurframe_->getTwc() after the motion model); the library inverts nothing.
 *   pose set   the slots i < n_h[b] with (status[i] & 3) == 1 && is3d[i], in slot order; m of them (mapkps_ after kltTracking removed
 *              the lost keypoints, restricted to is3d_).  k_pose_select writes that predicate as one byte per slot and k_pose_pack
 *              reads the byte (csrc/framepose.hip).
 *   inputs     of the chain, packed: unpx = the float unpx of the step's computeKeypoint widened to double, wpt = the slot's map
 *              point, scale = input->scale_h (NULL: all 0), bv = the step's bearing, Twc = input->Twc_h, p3p_req =
 *              input->p3p_req_h[b] || the step's own 33 % rule (:225-230), do_p3p = p3p_req || params->dop3p, samples = the table
 *              ov2_p3p_draw_samples(input->seed_h[b], m, params->n_rows, .) gives, drawn ON THE DEVICE, when do_p3p && m >= 4 (no
 *              table otherwise).
 *   result     results[b] is, to the last bit, what ov2_compute_pose returns on those inputs, EXCEPT that results[b].removed holds
 *              n_h[b] bytes IN SLOT SPACE: removed[i] speaks of slot i (0 kept or not in the pose set, 1 removed after P3P, 2
 *              removed after an accepted PnP).  results[b].removed must be non-NULL where n_h[b] > 0.
 *   nothing    On the first frame of a tracker and on a step where nothing is tracked (n_total == 0) no chain runs: action =
 *   ran        OV2_POSE_TOO_FEW, Twc = Twc_h, p3p_req_out = p3p_req_h[b], every other field (and removed) 0.
 * The 33 % rule stays on the host: it re-tracks the item's prior keypoints (ov2_fb_klt), which changes that item's positions and
 * status AFTER the device chain has run.  For an item where the rule fires, _end discards the device pose, rebuilds the pose set
 * from the final status / unpx / bv and runs ov2_compute_pose_batch over just those items with do_p3p = p3p_req = 1 and a table drawn
 * from the new m: a second submission with its own upload, six launches and synchronisation (the cost of one ov2_compute_pose_batch
 * call over the items concerned, on top of the retry's own ov2_fb_klt calls).  It is the rare path: a frame whose motion model
 * failed.
 * ov2_btracker_track_frame_end on a step begun with _pose_begin finishes the tracking half and drops the pose.
 *
 * NOT in the step: epipolar2d2dFiltering between tracking and pose (the shipped parameter files set doepipolar: 1; a caller with it
 * on keeps the route of separate calls: tracking, ov2_epipolar_filter_batch -- the function as one device chain, built on a
 * caller-owned block so that it can go between the select and the pack later --, ov2_compute_pose_batch), checkNewKfReq, the motion
 * model, kltTrackingFromKF.  (Since f18 the filter has a step of its own form: ov2_btracker_track_frame_epi_pose below puts that
 * chain between the select and the pack; this step is unchanged and remains the one for doepipolar: 0.  Since f19 the motion model
 * and checkNewKfReq run around either step in ov2_btracker_track_mono, at the end of this header.)
 *
 * OV2_EINVAL, checked on the host before anything is enqueued (the tracker stays where it was; the same frames can be passed
 * again): everything ov2_btracker_track_frame_map refuses; no calibration; NULL params / input / Twc_h / p3p_req_h / seed_h;
 * whatever ov2_compute_pose_batch refuses in params->pose; n_rows < 0 or > OV2_P3P_MAX_ROWS; cfg.n_max > OV2_P3P_MAX_POINTS;
 * |scale| > 60; a non-finite Twc_h; a non-finite wpt on an is3d slot of an active item.  unpx and bv are produced on the device
 * and CANNOT be checked on the host: the chain's own finiteness tests decide for them (k_pose_gather rejects a search whose
 * translation is not finite, k_pose_decide a PnP pose whose translation is not finite; the trust-region loop fails on a non-finite
 * step), so a non-finite bearing yields a refused pose, never an error code.
 * The pose buffers belong to the tracker: allocated by the first pose step (about 142 B per point slot and 121 B per sample row
 * of the whole batch), freed with the tracker. */
typedef struct {
    ov2_pose_params pose;        /* exactly what ov2_compute_pose takes (pnp, p3p, mono)                                     */
    int dop3p;                   /* SlamParams::dop3p_                                                                       */
    int n_rows;                  /* rows of the sample table drawn for an item that searches                                 */
} ov2_frame_pose_params;
typedef struct {                 /* per step; items / slots laid out like the map form's arrays                              */
    const double *Twc_h;         /* 7 per item: pcurframe_->getTwc() after the motion model                                  */
    const int *scale_h;          /* n_max per item: Keypoint::scale_; NULL = all 0                                           */
    const uint8_t *p3p_req_h;    /* 1 per item: bp3preq_ as it stands before this frame                                      */
    const unsigned long long *seed_h;  /* 1 per item: seed of the sample table                                               */
} ov2_frame_pose_input;
int  ov2_btracker_track_frame_pose_begin(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride, const float *kps_xy_h,
                                         const double *wpt_h, const uint8_t *is3d_h, const double *Tcw_h, const int *n_h,
                                         int klt_use_prior, const ov2_frame_pose_params *params, const ov2_frame_pose_input *input);
/* results: n_active of them (those of the step begun); p3p_req: the rule's flags as ov2_btracker_track_frame_end returns them */
int  ov2_btracker_track_frame_pose_end(ov2_btracker *t, float *out_xy_h, uint8_t *status_h, int *p3p_req, ov2_pose_result *results);
int  ov2_btracker_track_frame_pose(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride, const float *kps_xy_h,
                                   const double *wpt_h, const uint8_t *is3d_h, const double *Tcw_h, const int *n_h, int klt_use_prior,
                                   const ov2_frame_pose_params *params, const ov2_frame_pose_input *input,
                                   float *out_xy_h, uint8_t *status_h, int *p3p_req, ov2_pose_result *results);
/* What the last pose step fed the chain for `item` (for an item the rule re-ran: what the second run used): *m, the slot of each
 * packed point (m ints; slot_idx may be NULL), the sample table actually used (4 * *n_rows_used ints; samples may be NULL; 0 rows
 * when the item did not search).  slot_idx needs cfg.n_max ints of room, samples 4 * n_rows.  Reads the tracker's device buffers:
 * a diagnostic, not a per-frame call.  OV2_EINVAL before the first finished pose step. */
int  ov2_btracker_last_pose_inputs(const ov2_btracker *t, int item, int *m, int *slot_idx, int *samples, int *n_rows_used);

/* The lock-step step with epipolar2d2dFiltering AND the per-frame pose fused in (f18): what VisualFrontEnd::trackMono does per frame
 * with doepipolar_ == 1 (src/visual_front_end.cpp:86-116: kltTracking, epipolar2d2dFiltering, computePose), one enqueue and one
 * synchronisation (in _end), nothing visiting the host between tracking and pose.  A caller whose parameter file sets doepipolar: 1
 * -- every shipped one -- takes this step in place of the three separate calls.
 *
 * The keyframe the filter joins against (pmap_->map_pkfs_.at(pcurframe_->kfid_)) is RESIDENT ON THE DEVICE: it changes only when a
 * keyframe is created and does not travel with the steps.  ov2_btracker_set_keyframe gives item `item` its keyframe: kf_lmid
 * (n_kf, strictly ascending), kf_unpx (2 per entry), kf_bv (3 per entry), kf_Twc[7] -- the keyframe fields of ov2_epifilter_item,
 * validated on the host as ov2_epipolar_filter_batch validates them (NULL arrays with n_kf > 0, n_kf < 0, unsorted ids, bearings or
 * a pose that are not finite), plus n_kf <= cfg.n_max.  kf_Tcw is kf_Twc inverted on the host by ov2_se3_inverse (below); a caller
 * of the separate route that wants the step's bits passes that inverse as ov2_fkf_item.kf_Tcw.  The call copies on the context's
 * stream into the tracker's epipolar block and returns when the copy is done; it keeps a host copy (the rare path below reads it).
 * n_kf == 0 (kf_Twc may then be NULL) takes the keyframe away.  OV2_EINVAL between _begin and _end of any step.  An item without a
 * keyframe behaves as n_kf = 0: empty join, NaN parallax, OV2_EPIF_NO_MODEL, nothing removed (the reference returns early on a null
 * keyframe).  The block is allocated by the first set_keyframe or the first such step and freed with the tracker (about 119 B per
 * point slot -- 98 in the filter's block, 8 for the pack's lists, 13 pinned --, 36 B per keyframe slot, 137 B per sample row, 0.9 KB
 * per item); the context's scratch is not used.
 *
 * Per active item b, behind k_compute_keypoints on the context's stream:
 *   k_pose_select   as f16.
 *   k_epif_pack     (csrc/frameepi.hip) the slots i < n_h[b] with (status[i] & 3) == 1, in slot order -- the frame's keypoints after
 *                   kltTracking removed the lost ones -- into the filter's current-frame arrays: lmid = input->lmid_h, unpx = the
 *                   step's float unpx, bv = the step's bearing, is3d = the step's is3d_h; the item's record with nb3dkps = -1 (the
 *                   chain counts the flags of the packed frame: pcurframe_->nb3dkps_ after the removals), nbkfs and seed from the
 *                   input, cur_Twc = input->pose.Twc_h, the keyframe from the resident header.
 *   the chain       of ov2_epipolar_filter, its five launches untouched.
 *   k_epif_apply    removed (0 / 1 / 2), err and pair_cur from packed space to SLOT SPACE, and the select byte of every removed slot
 *                   cleared: the reference erases the RANSAC outliers from the frame before computePose reads it (:587-590; the
 *                   Sampson removals are 2-D keypoints and never were in the pose set).
 *   k_pose_pack, computePose's chain, k_pose_unpack   as f16: the pose set, m, the m >= 4 test and P3P's table are those of the
 *                   frame AFTER the filter.
 * epi_results[b] is, bit for bit, what ov2_epipolar_filter returns for those inputs, EXCEPT that removed holds n_h[b] bytes in slot
 * space, and err (n_h[b] floats) and pair_cur (pair_cur[k]: the slot of match k), where non-NULL, are in slot space too.
 * trace_samples must be NULL (ov2_btracker_last_epi_inputs fetches the table).  pose_results[b] is what ov2_compute_pose returns on
 * the filtered set, removed in slot space as f16.  status_h and out_xy_h are the tracking's, untouched by the filter.
 * On the first frame of a tracker and on a step where nothing is tracked no chain runs: the epipolar record is action =
 * OV2_EPIF_TOO_FEW_KPS with every other field (and removed, err) 0, the pose record is f16's.
 *
 * The 33 % rule stays on the host as in f16: for an item where it fires, _end discards BOTH device results, rebuilds the frame from
 * the final status / unpx / bv and runs ov2_epipolar_filter_batch (with the keyframe's host copy) and then ov2_compute_pose_batch
 * (do_p3p = p3p_req = 1) over just those items.
 * THE ONE DEVIATION from the reference: the mono branch do_optimize (:594).  pose_from_model and Twc_model are reported from the
 * UNREFINED model as ov2_epipolar_filter reports them, and the pose chain starts from the caller's Twc_h, never from Twc_model:
 * OpenGV's non-linear refinement has no device form.  Everything else is the reference's per-frame sequence.
 * ov2_btracker_track_frame_end on such a step finishes the tracking half and drops both results.
 *
 * OV2_EINVAL, checked on the host before anything is enqueued: everything ov2_btracker_track_frame_pose_begin refuses; whatever
 * ov2_epipolar_filter_batch refuses in params->epi (boptimize != 0 included); NULL lmid_h / nbkfs_h / epi_seed_h; epi.n_rows
 * outside [0, OV2_EPI_MAX_ROWS]; cfg.n_max > OV2_FKF_MAX_POINTS.  In _end: a NULL result array, a NULL `removed` where n_h[b] > 0, a
 * non-NULL trace_samples, a step that was not begun with _epi_pose_begin. */
typedef struct {
    ov2_frame_pose_params pose;  /* as f16                                                                                   */
    ov2_epifilter_params  epi;   /* as ov2_epipolar_filter_batch; epi.epi.boptimize must be 0                                */
} ov2_frame_epi_pose_params;
typedef struct {
    ov2_frame_pose_input pose;   /* as f16                                                                                   */
    const int *lmid_h;           /* n_max per item: Keypoint::lmid_ of each slot                                             */
    const int *nbkfs_h;          /* 1 per item: pmap_->nbkfs_                                                                */
    const unsigned long long *epi_seed_h;   /* 1 per item: seed of the 5-point sample table                                  */
} ov2_frame_epi_pose_input;
int  ov2_btracker_set_keyframe(ov2_btracker *t, int item, int n_kf, const int *kf_lmid, const float *kf_unpx, const double *kf_bv,
                               const double *kf_Twc);
int  ov2_btracker_track_frame_epi_pose_begin(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride,
                                             const float *kps_xy_h, const double *wpt_h, const uint8_t *is3d_h, const double *Tcw_h,
                                             const int *n_h, int klt_use_prior, const ov2_frame_epi_pose_params *params,
                                             const ov2_frame_epi_pose_input *input);
int  ov2_btracker_track_frame_epi_pose_end(ov2_btracker *t, float *out_xy_h, uint8_t *status_h, int *p3p_req,
                                           ov2_epifilter_result *epi_results, ov2_pose_result *pose_results);
int  ov2_btracker_track_frame_epi_pose(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride, const float *kps_xy_h,
                                       const double *wpt_h, const uint8_t *is3d_h, const double *Tcw_h, const int *n_h,
                                       int klt_use_prior, const ov2_frame_epi_pose_params *params,
                                       const ov2_frame_epi_pose_input *input, float *out_xy_h, uint8_t *status_h, int *p3p_req,
                                       ov2_epifilter_result *epi_results, ov2_pose_result *pose_results);
/* What the last such step fed the filter for `item` (for an item the rule re-ran: what the second run used): *n_cur and the slot of
 * each keypoint of the packed frame (n_cur ints; slot_idx may be NULL, else cfg.n_max ints of room), *m matches, the sample table
 * the search used (8 * *n_rows_used ints; samples may be NULL, else 8 * epi.n_rows ints of room; 0 rows when the item did not
 * search).  Reads the tracker's device buffers: a diagnostic, not a per-frame call.  OV2_EINVAL before the first finished step. */
int  ov2_btracker_last_epi_inputs(const ov2_btracker *t, int item, int *n_cur, int *slot_idx, int *m, int *samples, int *n_rows_used);
/* out = the inverse of the transform T, both [tx ty tz qx qy qz qw]: the conjugate quaternion and minus the rotated translation, the
 * rotation matrix of the conjugate written out, each sum of three terms serial.  Host arithmetic, no context. */
int  ov2_se3_inverse(const double T[7], double out[7]);

/* The constant-velocity MotionModel of the reference (include/visual_front_end.hpp:38-90) on the device (f19, csrc/motion.hip): the
 * two lines of VisualFrontEnd::trackMono that stand in front of and behind the per-frame step.  Fp64, one lane per item, Sophus'
 * SE(3) product, inverse, log and exp in the one device copy the pose-graph solver uses (csrc/se3_dev.hpp).  Poses are
 * [tx ty tz qx qy qz qw]; a pose is read as Sophus::SE3d(q, t) reads it (the quaternion normalised) and copied as it is given.
 *
 * The state is MotionModel's three members.  reset(): prev_time = -1, log_relT = 0 (prevTwc any finite pose).
 *
 * ov2_motion_apply: applyMotionModel(Twc, time) (:43-58).
 *   prev_time > 0:  d = (Twc * prevTwc^-1).log(); if NOT every |d_k| <= 1e-5 (Eigen's isZero(1.e-5) per coefficient; a NaN
 *                   coefficient is "not zero"), state_out.prevTwc = Twc_in and *resynced = 1 -- the estimator or the loop closer
 *                   moved the frame since the last update.  Twc_out = Twc * exp(log_relT * (time - prev_time)).
 *   otherwise:      Twc_out = Twc_in, *resynced = 0.
 *   state_out is state_in but for that prevTwc.  Tcw_out is Twc_out inverted in the arithmetic of ov2_se3_inverse -- products, sums
 *   and negations, compiled without contraction on both sides --, so it equals ov2_se3_inverse(Twc_out) BIT FOR BIT.
 * ov2_motion_update: updateMotionModel(Twc, time) (:60-78).
 *   prev_time < 0:  only stores: prev_time = time, prevTwc = Twc.
 *   otherwise:      log_relT = (prevTwc^-1 * Twc).log() / (time - prev_time), prev_time = time, prevTwc = Twc.
 * (prev_time == 0 is the reference's own gap between "> 0" and "< 0": apply leaves the pose, update takes the second branch.)
 * Device sin / cos / atan are not libm's: against tests/motion_ref.py the doubles agree to rounding (tests/test_gpu_motion.py holds
 * them to the rule of the pose-graph tests), resynced exactly wherever no |d_k| sits on the threshold.
 *
 * The batch forms take n items (state_in, time: n; Twc: 7 n; resynced: n bytes) in one upload, one launch, one download and one
 * synchronisation on the context's stream; the single forms are the batch of one.  Outputs may alias the inputs.  n == 0: OV2_OK.
 * OV2_EINVAL, checked on the host before the context is touched, nothing written: n < 0; a NULL array; a state, pose or time that is
 * not finite; prev_time >= 0 && time <= prev_time (the reference exits on dt < 0 and divides by zero on dt == 0: both are refused,
 * by apply as by update).  Finite inputs with dt > 0 give a finite log and exp, so the outputs are finite. */
typedef struct {
    double prev_time;            /* MotionModel::prev_time_; < 0: no pose stored yet                                         */
    double prevTwc[7];           /* MotionModel::prevTwc_                                                                    */
    double log_relT[6];          /* MotionModel::log_relT_: [upsilon; omega] per second                                      */
} ov2_motion_state;
int  ov2_motion_apply(ov2_ctx *ctx, const ov2_motion_state *state_in, const double Twc_in[7], double time,
                      ov2_motion_state *state_out, double Twc_out[7], double Tcw_out[7], uint8_t *resynced);
int  ov2_motion_apply_batch(ov2_ctx *ctx, int n, const ov2_motion_state *state_in, const double *Twc_in, const double *time,
                            ov2_motion_state *state_out, double *Twc_out, double *Tcw_out, uint8_t *resynced);
int  ov2_motion_update(ov2_ctx *ctx, const ov2_motion_state *state_in, const double Twc[7], double time, ov2_motion_state *state_out);
int  ov2_motion_update_batch(ov2_ctx *ctx, int n, const ov2_motion_state *state_in, const double *Twc, const double *time,
                             ov2_motion_state *state_out);

/* The lock-step step that IS VisualFrontEnd::trackMono after initialisation (f19; src/visual_front_end.cpp:65-128): the motion model
 * in front of the step of f18 (doepipolar: 1) or f16 (doepipolar: 0), and behind it updateMotionModel and checkNewKfReq, one enqueue
 * and one synchronisation.  The caller hands over images, keypoints, map points and a timestamp and gets the tracked frame, the
 * filter's record, the pose and the keyframe request; it does no pose arithmetic.  What remains with it per frame is the map (which
 * slots exist) and createKeyframe.  (Since f20 createKeyframe has a lock-step form too: ov2_btracker_create_keyframe, at the end of this
 * header, takes this step's kf.decision.)
 *
 * RESIDENT ON THE DEVICE per item, mirrored on the host: the frame pose (pcurframe_->Twc_; the identity at first), the
 * ov2_motion_state (reset() at first) and the keyframe's id_, img_time_ and nb3dkps_ next to the keyframe arrays of
 * ov2_btracker_set_keyframe.  ov2_btracker_set_pose: the estimator or the loop closer moved the frame -- the case applyMotionModel's
 * resync exists for; a non-finite pose is refused.  ov2_btracker_reset_motion: MotionModel::reset().  ov2_btracker_set_keyframe_info:
 * call it with ov2_btracker_set_keyframe.  The get_ calls return the mirrors.  All five return OV2_EINVAL between _begin and _end.
 *
 * params: the ov2_frame_epi_pose_params as they are (step.epi.fkf carries ncellsize, nbwcells, nbhcells, nbmaxkps, finit_parallax
 * and stereo for the decision) plus doepipolar; with doepipolar == 0 step.epi's search settings are not read, the filter is skipped
 * and epi_results must be NULL.  input: the ov2_frame_epi_pose_input with step.pose.Twc_h == NULL (there is no Tcw_h argument
 * either), plus time_h, frame_id_h and localba_is_on_h (NULL: all 0) per item; nbkfs_h / epi_seed_h may be NULL with doepipolar == 0.
 *
 * On the context's stream, nothing visiting the host:
 *   k_mono_apply    (csrc/mono.hip) ov2_motion_apply on the resident pose and state: the predicted Twc into the pose block, its
 *                   inverse into the map block -- behind those blocks' uploads, ahead of k_prior_frame.
 *   the step        of f18 (or f16), untouched: same kernels, same launches.
 *   k_mono_pack     the frame checkNewKfReq sees, in slot order: the slots with (status & 3) == 1 whose filter `removed` byte (either
 *                   kind) and pose `removed` byte are 0 -- none where the pose's action is OV2_POSE_P3P_RESET or OV2_POSE_PNP_RESET
 *                   (resetFrame(), :1181-1203) --, with lmid, the tracked px, unpx, bv and is3d; the item's record: cur_Twc = the pose
 *                   record's Twc, the keyframe's fields from the resident block, kf_Tcw the one set_keyframe derived, noccupcells =
 *                   nb3dkps = -1.  Its thread 0 runs ov2_motion_update on the pose record's Twc and stores the new resident pose
 *                   (that Twc) and state.
 *   k_fkf_parallax  itself (csrc/fkf.hip), as ov2_kf_decision_batch launches it.
 * Everything ov2_btracker_track_frame_epi_pose_end returns is returned as there; mono_results[b] adds the predicted Twc, resynced,
 * the state after the update and the decision -- byte for byte what ov2_motion_apply_batch, the step with that pose,
 * ov2_motion_update_batch and ov2_kf_decision_batch on the frame above return (tests/test_gpu_trackmono.py).
 * The tracker's first frame: nothing runs, as in f18; the pose record carries the resident pose, the decision record is zero with
 * decision = 1 and reason = OV2_KF_FIRST_FRAME (:77), the motion state is untouched.  Any later step: the motion model and the
 * decision run for every active item, also where an item or the whole step has no keypoints (computePose returns at :667, the
 * update stores, nb3dkps_ = 0 decides).  An item without a keyframe (n_kf == 0) or without keyframe info: the decision record is
 * zero with decision = 0 and reason = OV2_KF_NO_KEYFRAME (:994).
 * The 33 % rule stays on the host as in f16 / f18: for an item where it fires, _end re-runs the filter and the pose as there, then
 * ov2_motion_update_batch and ov2_kf_decision_batch over just those items from the state BEFORE the step's update, and writes the
 * corrected pose and state back into the resident block.  After _end the resident pose and state of every item are the route's.
 * ov2_btracker_track_frame_end on such a step gives the tracking half, drops the rest and puts the resident pose and state back.
 *
 * OV2_EINVAL, checked on the host before anything is enqueued: everything the step of f18 (f16) refuses except Twc_h / Tcw_h, which
 * are gone (a non-NULL Twc_h is refused); NULL lmid_h / time_h / frame_id_h; a time that is not finite or not after the item's
 * prev_time where that is >= 0; no calibration; the grid ov2_kf_decision refuses; cfg.n_max > OV2_FKF_MAX_POINTS.  A predicted pose
 * cannot be checked on the host any more; it is finite because the resident values are (set_pose refuses anything else, the
 * chain's own tests refuse a non-finite pose) and dt > 0, which give a finite log and exp. */
typedef struct {
    ov2_frame_epi_pose_params step;   /* as f18                                                                              */
    int doepipolar;                   /* SlamParams::doepipolar_: 1 the step of f18, 0 the step of f16                       */
} ov2_track_mono_params;
typedef struct {
    ov2_frame_epi_pose_input step;    /* as f18; step.pose.Twc_h must be NULL                                                */
    const double *time_h;             /* 1 per item: pcurframe_->img_time_                                                   */
    const int *frame_id_h;            /* 1 per item: pcurframe_->id_                                                         */
    const uint8_t *localba_is_on_h;   /* 1 per item: pslamstate_->blocalba_is_on_; NULL = all 0                              */
} ov2_track_mono_input;
typedef struct {
    double Twc_pred[7];               /* the pose after applyMotionModel: what tracking and the pose chain started from      */
    int resynced;                     /* applyMotionModel moved prevTwc_ to the frame pose                                   */
    ov2_motion_state state;           /* after updateMotionModel                                                             */
    ov2_kf_decision_result kf;        /* checkNewKfReq                                                                       */
} ov2_track_mono_result;
int  ov2_btracker_set_pose(ov2_btracker *t, int item, const double Twc[7]);
int  ov2_btracker_get_pose(ov2_btracker *t, int item, double Twc[7]);
int  ov2_btracker_reset_motion(ov2_btracker *t, int item);
int  ov2_btracker_get_motion(ov2_btracker *t, int item, ov2_motion_state *state);
int  ov2_btracker_set_keyframe_info(ov2_btracker *t, int item, int kf_id, double kf_time, int kf_nb3dkps);
int  ov2_btracker_track_mono_begin(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride, const float *kps_xy_h,
                                   const double *wpt_h, const uint8_t *is3d_h, const int *n_h, int klt_use_prior,
                                   const ov2_track_mono_params *params, const ov2_track_mono_input *input);
int  ov2_btracker_track_mono_end(ov2_btracker *t, float *out_xy_h, uint8_t *status_h, int *p3p_req, ov2_epifilter_result *epi_results,
                                 ov2_pose_result *pose_results, ov2_track_mono_result *mono_results);
int  ov2_btracker_track_mono(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride, const float *kps_xy_h,
                             const double *wpt_h, const uint8_t *is3d_h, const int *n_h, int klt_use_prior,
                             const ov2_track_mono_params *params, const ov2_track_mono_input *input, float *out_xy_h, uint8_t *status_h,
                             int *p3p_req, ov2_epifilter_result *epi_results, ov2_pose_result *pose_results,
                             ov2_track_mono_result *mono_results);

/* MapManager::createKeyframe for the items of a lock-step batch that were asked to become keyframes (f20; src/map_manager.cpp:44-61,
 * :286-362): what VisualFrontEnd::visualTracking does after trackMono returned true, in ONE enqueue on the context's stream and ONE
 * synchronisation, with nothing visiting the host in between.  It replaces, per keyframe round, ov2_btracker_describe_brief of the
 * frame, the occupied-cell count, ov2_btracker_detect_singlescale / _grid_fast, ov2_btracker_describe_brief of the new points,
 * ov2_compute_keypoints, a sort by lmid on the host and ov2_btracker_set_keyframe + ov2_btracker_set_keyframe_info ONCE PER ITEM --
 * and returns byte for byte what that route returns and installs (tests/test_gpu_createkf.py; tests/createkf_ref.py is the route).
 *
 * input, in slot layout with cfg.n_max slots per item: px_h / lmid_h / is3d_h / n_h are the current frame AFTER all of the step's
 * removals and after prepareFrame.  prepareFrame's filter (:267-284) walks vgridkps_ in insertion order and needs the map's
 * observation counts, so it stays with the caller.  make_kf_h: one byte per item, normally mono_results[b].kf.decision.  nlmid_h:
 * MapManager::nlmid_ per item; nkfid_h / time_h: the id and img_time_ the keyframe gets.  Twc_h: 7 doubles per item, NULL: the
 * resident pose of f19.  quality_inout (single scale) or fast_th_inout (grid FAST): the per-item adaptive state; the pointer must
 * stay valid until _end, which updates it.
 *
 * Per flagged item, on the device, in the reference's order:
 *   k_ckf_prepare   (csrc/createkf.hip) noccupcells as Frame::addKeypointToGrid leaves it -- Frame::getKeypointCellIdx on the grid of
 *                   params, the counting of ov2_kf_decision -- and nb3dkps from is3d; nb2detect = nbmaxkps - noccupcells.
 *   detection       if nb2detect > 0: detectSingleScale / detectGridFAST on level 0 of the current pyramid with the frame's
 *                   keypoints as the occupied set -- the three launches of the detectors with cell det_cell, the count left on the
 *                   device.  An item that is not flagged or has nb2detect <= 0 carries a skip byte: its work-groups leave at once.
 *   k_ckf_append    addKeypointsToFrame: the new points behind slot n_prev in the detector's output order, lmid = nlmid + k,
 *                   is3d = 0, colour = level 0 at ((int)y, (int)x).
 *   computeKeypoint unpx / bv of ALL slots of the new frame (k_compute_keypoints); needs ov2_btracker_set_calibration.
 *   describeBRIEF   with use_brief != 0: k_brief32 over the n_prev + n_new points on the step's RAW frame, under the conditions of
 *                   ov2_btracker_describe_brief (an invalid descriptor: 32 zero bytes, valid = 0).  use_brief == 0: no BRIEF runs.
 *   k_ckf_install   addKeyframe as far as the tracker holds it: lmid / unpx / bv sorted strictly ascending by lmid into the arrays
 *                   ov2_btracker_set_keyframe writes, the header {n_kf, kf_Twc, its inverse}, {nkfid, nb3dkps, has_info = 1} and
 *                   time where ov2_btracker_set_keyframe_info writes.  The new frame becomes the item's resident keyframe without
 *                   leaving the device; _end brings the host mirrors (the 33 % rule's re-run, the get_ calls) to the same state.
 * The tracker's first frame (n_h = 0 everywhere) runs all of it on empty frames.
 *
 * results[b].action:
 *   OV2_CKF_NOT_REQUESTED  make_kf_h[b] == 0.  Nothing of the item is written but this action: the resident keyframe, its info, the
 *                          adaptive state and the output slots are untouched.
 *   OV2_CKF_CREATED        the record is complete; slots [0, n_kf) of out_px_h / out_lmid_h / unpx_h / bv_h (and desc_h / valid_h
 *                          with use_brief) hold the new frame in slot order, slots [n_prev, n_kf) of color_h the new points' colour.
 *   OV2_CKF_OVERFLOW       n_prev + n_new > cfg.n_max.   } the record is filled (n_new is the true count), nothing else of the item
 *   OV2_CKF_DUP_LMID       lmid_h repeats an id.         } is written, the resident keyframe and its info stay as they were; the
 *                          caller falls back to the separate calls for that item.
 * The adaptive state is updated from the detector's counters by the reference's rules for every flagged item whose detection ran
 * (nb2detect > 0, also with OVERFLOW / DUP_LMID) and for no other item.
 *
 * OV2_EINVAL, checked on the host before anything is enqueued (the tracker stays where it was): NULL tracker / params / input /
 * px_h / lmid_h / is3d_h / n_h / make_kf_h / nlmid_h / nkfid_h / time_h / the detector's state array; n_active outside [1, batch] or
 * beyond the items of the current step; n_h[b] outside [0, cfg.n_max]; a step or another call of this kind open; no current raw
 * frames; no calibration; a grid ov2_kf_decision refuses or a cell the detectors refuse (OV2_EUNSUPPORTED where they say so);
 * cfg.n_max > OV2_FKF_MAX_POINTS; on a flagged item lmid_h[i] < 0 or >= nlmid_h[b] (the reference's counter is monotone), a
 * non-finite time_h / Twc_h; nlmid_h[b] + 2 * cells overflowing int; Twc_h == NULL on a tracker without a resident pose block;
 * detector OV2_CKF_DET_GFTT (detectGFTT is not fused); a mask_mode the detector refuses.  In _end: no open call, a NULL result array
 * or output array.  Between _begin and _end the calls that change the tracker's resident state or start a step return OV2_EINVAL. */
#define OV2_CKF_DET_SINGLESCALE 0
#define OV2_CKF_DET_GRID_FAST   1
#define OV2_CKF_DET_GFTT        2
enum { OV2_CKF_NOT_REQUESTED = 0, OV2_CKF_CREATED = 1, OV2_CKF_OVERFLOW = 2, OV2_CKF_DUP_LMID = 3 };
typedef struct {
    int ncellsize, nbwcells, nbhcells, nbmaxkps;   /* the frame's grid, as ov2_fkf_params carries it                          */
    int detector;                     /* OV2_CKF_DET_*                                                                       */
    int det_cell;                     /* the detector's cell size (nmaxdist_)                                                */
    int roi[4];                       /* single scale: x, y, w, h as ov2_detect_singlescale takes it                         */
    int mask_mode;                    /* grid FAST: OV2_MASK_*                                                               */
    int do_subpix;
    int use_brief;                    /* SlamParams::use_brief_                                                              */
} ov2_create_keyframe_params;
typedef struct {
    const float *px_h;                /* 2 per slot                                                                          */
    const int *lmid_h;                /* 1 per slot                                                                          */
    const uint8_t *is3d_h;            /* 1 per slot                                                                          */
    const int *n_h;                   /* 1 per item                                                                          */
    const uint8_t *make_kf_h;         /* 1 per item                                                                          */
    const int *nlmid_h;               /* 1 per item: MapManager::nlmid_                                                      */
    const int *nkfid_h;               /* 1 per item: the keyframe's id                                                       */
    const double *time_h;             /* 1 per item: img_time_                                                               */
    const double *Twc_h;              /* 7 per item; NULL: the resident pose                                                 */
    double *quality_inout;            /* 1 per item, single scale: dmaxquality_                                              */
    int *fast_th_inout;               /* 1 per item, grid FAST: nfast_th_                                                    */
} ov2_create_keyframe_input;
typedef struct {
    int action;                       /* OV2_CKF_*                                                                           */
    int n_prev, noccupcells, nb2detect, n_new, n_kf, nb3dkps;
    int pad;
} ov2_create_keyframe_result;
int  ov2_btracker_create_keyframe_begin(ov2_btracker *t, int n_active, const ov2_create_keyframe_params *params,
                                        const ov2_create_keyframe_input *input);
int  ov2_btracker_create_keyframe_end(ov2_btracker *t, ov2_create_keyframe_result *results, float *out_px_h, int *out_lmid_h,
                                      float *unpx_h, double *bv_h, uint8_t *desc_h, uint8_t *valid_h, uint8_t *color_h);
int  ov2_btracker_create_keyframe(ov2_btracker *t, int n_active, const ov2_create_keyframe_params *params,
                                  const ov2_create_keyframe_input *input, ov2_create_keyframe_result *results, float *out_px_h,
                                  int *out_lmid_h, float *unpx_h, double *bv_h, uint8_t *desc_h, uint8_t *valid_h, uint8_t *color_h);

/* The current frame RESIDENT ON THE DEVICE between the lock-step steps (f21): per item of an ov2_btracker the count n and per slot
 * px (2 float), lmid, is3d and the 3-D point wpt (3 double), mirrored on the host.  ov2_btracker_track_mono and
 * ov2_btracker_create_keyframe take the frame from the host at every call, and the caller rebuilds it between two calls by the rule
 * of k_mono_pack; with the calls below the tracker carries it, and the caller sends up only what the map changed.  The block is
 * double-buffered per item: a call reads an item's frame from one buffer and writes the next frame into the other, and its _end
 * decides which holds -- so ov2_btracker_track_frame_end on a resident step leaves the frame as it was before the step.
 *
 * ov2_btracker_set_frame    installs item's frame (first install, and the fallback after OV2_CKF_OVERFLOW / OV2_CKF_DUP_LMID or a
 *                           re-initialisation): one copy up, one synchronisation.
 * ov2_btracker_get_frame    from_device != 0: the device block copied down (one synchronisation); 0: the mirror.  Any output
 *                           pointer may be NULL; the arrays hold cfg.n_max slots, [0, *n) are written.  wpt of a slot with
 *                           is3d == 0 is whatever the slot last carried.
 * ov2_btracker_update_frame[_batch]   what the map did to the frames since the last step, as a list of ops per item -- the batch
 *                           form for items [0, n_active) (ops_h[b]: n_ops_h[b] ops; may be NULL where that is 0), the single
 *                           form for one item:
 *     OV2_RES_SET_POINT     triangulation, local BA or matchToMap gave or moved the 3-D point: wpt = xyz, is3d = 1
 *     OV2_RES_UNSET_POINT   is3d = 0 (the point is kept in the slot)
 *     OV2_RES_REMOVE        removeObsFromCurFrameById, prepareFrame's filter: the slot leaves the frame, the rest close up in slot
 *                           order
 *                           An lmid the frame does not hold is skipped and counted (n_missing).  One upload (the ops, packed), one
 *                           launch (k_res_update, csrc/resident.hip: a work-group per item, the list's ids in LDS), one download (the
 *                           records) and one synchronisation; the mirror is advanced on the host by the same rule.
 * ov2_btracker_track_mono_resident[_begin / _end]   ov2_btracker_track_mono on the resident frame: its arguments without kps_xy_h,
 *                           wpt_h, is3d_h and n_h; input->step.lmid_h and input->step.pose.scale_h must be NULL (every scale is 0).
 *                           k_res_stage writes the frame where the step's kernels read it -- the per-slot ranges are not copied up
 *                           --, the step of f19 runs untouched, and k_res_carry behind k_mono_pack writes the next frame by that
 *                           kernel's rule: the tracked px of the slots with (status & 3) == 1 whose filter byte and pose byte are 0,
 *                           with their lmid, is3d and wpt, in slot order; none where the pose's action is OV2_POSE_P3P_RESET or
 *                           OV2_POSE_PNP_RESET.  _end returns what ov2_btracker_track_mono_end returns, in the slot space of the
 *                           frame BEFORE the step, plus n_before / n_after per item (frame_results, may be NULL); the next frame
 *                           comes down with the results into the mirror.  Where the 33 % rule fired, _end rebuilds that item's
 *                           frame on the host from the second run's removals and copies that one item up.  The tracker's first
 *                           frame and a step with no keypoint anywhere leave every frame as it is; so does any step for the items
 *                           beyond n_active.  ov2_btracker_track_mono_end finishes a resident step too (without frame_results).
 * ov2_btracker_create_keyframe with input->px_h == NULL (lmid_h, is3d_h and n_h must then be NULL too) reads the resident frame:
 *                           k_res_ckf_in fills the call's input ranges on the device, and behind k_ckf_install k_res_adopt makes
 *                           the frame with the new points appended (is3d = 0, wpt = 0) the resident frame of every
 *                           OV2_CKF_CREATED item; an item that is NOT_REQUESTED, OVERFLOW or DUP_LMID keeps its frame.  Outputs and
 *                           the installed keyframe are those of the host form.
 * ov2_btracker_last_slot_bytes   the bytes of PER-SLOT input (any range whose size goes with n or cfg.n_max: keypoints, points,
 *                           flags, ids, scales; not images, not per-item scalars) that the last _begin of a step or of
 *                           create_keyframe wrote for the device: > 0 for the host forms with a non-empty frame, 0 for the
 *                           resident forms.
 *
 * OV2_EINVAL, checked on the host before anything is enqueued: a NULL tracker; an item or n_active out of range; an open step or
 * an open create_keyframe call (set_frame, get_frame and update_frame alike); cfg.n_max >
 * OV2_FKF_MAX_POINTS.  set_frame: n outside [0, cfg.n_max]; a NULL array with n > 0; a non-finite px; a non-finite wpt on an is3d
 * slot; a negative or repeated lmid.  update_frame: n_ops outside [0, cfg.n_max]; a NULL list with n_ops > 0; an unknown op; an
 * lmid repeated within one item's list; a non-finite xyz on OV2_RES_SET_POINT.  track_mono_resident: everything
 * ov2_btracker_track_mono refuses of the remaining arguments; a non-NULL lmid_h / scale_h; _end on a step that was not begun with
 * _resident_begin. */
#define OV2_RES_SET_POINT   0
#define OV2_RES_UNSET_POINT 1
#define OV2_RES_REMOVE      2
typedef struct {
    int lmid;                         /* the map point's id                                                                  */
    int op;                           /* OV2_RES_*                                                                           */
    double xyz[3];                    /* OV2_RES_SET_POINT: the point in the world frame; else unused                        */
} ov2_resident_op;
typedef struct {
    int n_before, n_after;            /* the frame's size                                                                    */
    int n_set, n_unset, n_removed;    /* ops applied, by kind                                                                */
    int n_missing;                    /* ops whose lmid the frame does not hold                                              */
} ov2_resident_update_result;
typedef struct {
    int n_before, n_after;            /* the frame's size before the step and after its removals                             */
} ov2_resident_step_result;
int  ov2_btracker_set_frame(ov2_btracker *t, int item, int n, const float *px, const int *lmid, const uint8_t *is3d, const double *wpt);
int  ov2_btracker_get_frame(ov2_btracker *t, int item, int from_device, int *n, float *px, int *lmid, uint8_t *is3d, double *wpt);
int  ov2_btracker_update_frame(ov2_btracker *t, int item, int n_ops, const ov2_resident_op *ops, ov2_resident_update_result *result);
int  ov2_btracker_update_frame_batch(ov2_btracker *t, int n_active, const int *n_ops_h, const ov2_resident_op *const *ops_h,
                                     ov2_resident_update_result *results);
int  ov2_btracker_track_mono_resident_begin(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride, int klt_use_prior,
                                            const ov2_track_mono_params *params, const ov2_track_mono_input *input);
int  ov2_btracker_track_mono_resident_end(ov2_btracker *t, float *out_xy_h, uint8_t *status_h, int *p3p_req,
                                          ov2_epifilter_result *epi_results, ov2_pose_result *pose_results,
                                          ov2_track_mono_result *mono_results, ov2_resident_step_result *frame_results);
int  ov2_btracker_track_mono_resident(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride, int klt_use_prior,
                                      const ov2_track_mono_params *params, const ov2_track_mono_input *input, float *out_xy_h,
                                      uint8_t *status_h, int *p3p_req, ov2_epifilter_result *epi_results, ov2_pose_result *pose_results,
                                      ov2_track_mono_result *mono_results, ov2_resident_step_result *frame_results);
int  ov2_btracker_last_slot_bytes(const ov2_btracker *t, size_t *h2d);

/* The mapper's STEREO block on the resident keyframe (f22): what Mapper::run executes on every new stereo keyframe
 * (src/mapper.cpp:69-105) -- MapManager::stereoMatching (src/map_manager.cpp:367-611), then Mapper::triangulateStereo
 * (src/mapper.cpp:346-461) -- for the items ov2_btracker_create_keyframe just turned into keyframes, in ONE enqueue on the context's
 * stream and ONE synchronisation, byte-equal to the route of separate calls (ov2_btracker_get_frame, ov2_compute_keypoints,
 * ov2_stereo_priors_batch, ov2_stereo_match_batch, ov2_compute_keypoints of the right camera, ov2_triangulate_keyframe_batch,
 * ov2_btracker_update_frame_batch, ov2_btracker_set_keyframe_info).  Per item b of [0, n_active) with do_h[b] != 0 whose resident
 * frame is its resident keyframe, in the reference's order (csrc/stereokf.hip between the existing kernels):
 *   input      k_skf_input: from the resident frame px, lmid, is3d, wpt and n, from the resident keyframe header its Twc and Tcw as
 *              k_ckf_install wrote them.  state = is3d: state 2 (a 3-D keypoint whose map point is gone, :415-418) CANNOT OCCUR
 *              here -- the caller removes such observations with ov2_btracker_update_frame first.  unpx / bv of every slot by the
 *              left camera of ov2_btracker_set_calibration (the bits of ov2_compute_keypoints), the keypoint on the coarsest
 *              level, the per-item descriptors of the kernels behind (0 for an item that is not OV2_SKF_DONE).  With rect == 0
 *              the keypoint grid of Frame::getSurroundingKeypoints: ceil(img_w / ncellsize) x ceil(img_h / ncellsize) cells, a
 *              keypoint in cell (floorf(px.y / cellsize), floorf(px.x / cellsize)) as k_prior_stereo computes it, a keypoint
 *              outside the grid in none.  KEYPOINTS INSIDE A CELL STAND IN SLOT ORDER.  The reference's order is vgridkps_
 *              insertion order, which depends on the frame's history and is not carried by the resident frame: the one
 *              deviation.  It changes only the summation order of the neighbour-depth prior, a starting point for LK.
 *   priors     k_prior_stereo (ov2_stereo_priors), then k_skf_seed: prior = has_prior ? prior : px, flag = has_prior != 0
 *   matching   k_line_min_sad on level nklt_pyr_lvl (rect) or "nothing found", k_track_klt from the tracker's current pyramid into
 *              `right`, k_epipolar_check with the right camera: the grids and arguments of ov2_stereo_match_batch
 *   keypoints  k_skf_stereo_kp: stereo_ok = tracked && gate; right_px as ov2_stereo_match_batch returns it ((0, 0) where the
 *              tracking failed, the corrected row for rect); for stereo_ok slots runpx / rbv by the right camera's computeKeypoint
 *              on right_px (Frame::computeStereoKeypoint, frame.cpp:405-420); is_stereo = stereo_ok && !is3d (mapper.cpp:383)
 *   triangulation   k_triangulate with src = -1 everywhere: the stereo pass alone.  Mapper::triangulateTemporal is the call behind
 *              this one, ov2_btracker_temporal_keyframe (it needs the source keyframes: the tracker's anchor table).
 *              updateMapPoint's other effects and removeStereoKeypointById's bookkeeping are OUT OF SCOPE: the statuses
 *              returned are what a caller needs to replay them.
 *   apply      k_skf_apply: every OV2_TRI_STEREO_OK slot gets is3d = 1 and wpt = the triangulated point, written into the item's
 *              OTHER frame buffer (_end flips it: a call begun and never ended leaves the frame as it was); kf_nb3dkps of the
 *              resident keyframe info becomes the number of is3d slots after the call (updateMapPoint -> turnKeypoint3d on the
 *              keyframe's nb3dkps_, which checkNewKfReq reads).  _end brings the host mirrors of the frame and of the info to the
 *              same state from the statuses and points that come down anyway.
 * `right`: a batch pyramid of the right images built by the caller on the tracker's context (ov2_pyr_build_clahe_hb / ov2_pyr_build_h,
 * as for ov2_stereo_match_batch), at least n_active items, of the tracker's size, window and level count; it may still be building
 * on that stream.  The tracker owns no right pyramid.  The left camera is that of ov2_btracker_set_calibration.
 * results[b].action:
 *   OV2_SKF_NOT_REQUESTED   do_h[b] == 0: nothing of the item is read or written, its work-groups leave at once
 *   OV2_SKF_NOT_KEYFRAME    the item's resident frame is not its resident keyframe: nothing is written.  The tracker keeps one
 *                           host byte per item: set by the _end of a resident ov2_btracker_create_keyframe whose action was
 *                           OV2_CKF_CREATED; cleared by ov2_btracker_set_frame, ov2_btracker_set_keyframe, any resident step's _end
 *                           that flipped the item, and an ov2_btracker_update_frame that removed a slot
 *   OV2_SKF_DONE            the record and, in the slot space of the resident frame (cfg.n_max slots per item, [0, n) written),
 *                           right_px_h (2 float), stereo_ok_h, tri_status_h (OV2_TRI_* bits), wpt_h (3 double), invdepth_h
 * ov2_btracker_last_slot_bytes reports 0 after this call.  ov2_btracker_get_keyframe_info returns the resident keyframe info of
 * an item (from_device != 0: copied down, one synchronisation; else the host mirror); any output pointer may be NULL.
 * OV2_EINVAL, checked on the host before anything is enqueued (the tracker stays where it was): a NULL tracker / params / right /
 * do_h; n_active outside [1, batch]; `right` with fewer items than n_active or another size, window or level count than the
 * tracker's pyramid; an open step, create_keyframe call or call of this kind; no calibration; no resident block; cfg.n_max >
 * OV2_FKF_MAX_POINTS; rect == 0 with ncellsize <= 0 or more than OV2_FKF_MAX_CELLS cells; params->tri.stereo == 0; a non-finite
 * pose in Tcic0 / tri.Tcic0 / tri.Tlr; the camera checks of ov2_stereo_priors (OV2_EUNSUPPORTED where it says so).  _end: no open
 * call, a NULL result or output array.  Between _begin and _end the calls that change resident state or start a step return
 * OV2_EINVAL. */
#define OV2_SKF_NOT_REQUESTED 0
#define OV2_SKF_NOT_KEYFRAME  1
#define OV2_SKF_DONE          2
typedef struct {
    int nklt_win_size;                /* ov2_stereo_match_batch: nklt_win_size_                                              */
    int nklt_pyr_lvl;                 /* ov2_stereo_match_batch: nklt_pyr_lvl_                                               */
    int max_iter;                     /* ov2_stereo_match_batch: nmax_iter_                                                  */
    float eps;                        /* ov2_stereo_match_batch: fmax_px_precision_                                          */
    float nklt_err;                   /* ov2_stereo_match_batch: nklt_err_                                                   */
    float fmax_fbklt_dist;            /* ov2_stereo_match_batch: fmax_fbklt_dist_                                            */
    int rect;                         /* ov2_stereo_priors_params.rect / ov2_stereo_match_batch: bdo_stereo_rect_            */
    double Frl[9];                    /* ov2_stereo_match_batch: the fundamental matrix of the gate (read when rect == 0)    */
    int model;                        /* ov2_stereo_priors_params / ov2_compute_keypoints: the RIGHT camera's model          */
    double K[4];                      /* ov2_stereo_priors_params / ov2_compute_keypoints: right fx fy cx cy                 */
    const double *D;                  /* ov2_stereo_priors_params / ov2_compute_keypoints: right distortion vector, or NULL  */
    int nD;                           /* ov2_stereo_priors_params / ov2_compute_keypoints: its length (0: none)              */
    double iK[9];                     /* ov2_compute_keypoints of the right camera: its iK_, row-major                       */
    double img_w, img_h;              /* ov2_stereo_priors_params: pcalib_rightcam_->img_w_ / img_h_, the size behind the grid */
    double Tcic0[7];                  /* ov2_stereo_priors_params: pcalib_rightcam_->Tcic0_                                  */
    int ncellsize;                    /* ov2_stereo_priors_params: Frame::ncellsize_ (read when rect == 0)                   */
    ov2_tri_params tri;               /* ov2_triangulate_keyframe_batch: its params, as they are (tri.stereo must be set)    */
} ov2_stereo_keyframe_params;
typedef struct {
    int action;                       /* OV2_SKF_*; the other fields are 0 unless OV2_SKF_DONE                               */
    int n;                            /* the frame's size                                                                    */
    int n_prior3d, n_prior_nb;        /* ov2_stereo_priors_result: priors of kind 1 / kind 2                                 */
    int n_stereo_kps;                 /* stereo_ok slots: the reference's nb_stereo_kps_ after stereoMatching                */
    int n_stereo, n_stereo_good;      /* ov2_tri_result: nbstereo / good of triangulateStereo                                */
    int nb3dkps;                      /* is3d slots of the frame after the call: the keyframe info's kf_nb3dkps              */
} ov2_stereo_keyframe_result;
int  ov2_btracker_stereo_keyframe_begin(ov2_btracker *t, int n_active, const ov2_stereo_keyframe_params *params,
                                        const ov2_pyr *right, const uint8_t *do_h);
int  ov2_btracker_stereo_keyframe_end(ov2_btracker *t, ov2_stereo_keyframe_result *results, float *right_px_h,
                                      uint8_t *stereo_ok_h, uint8_t *tri_status_h, double *wpt_h, double *invdepth_h);
int  ov2_btracker_stereo_keyframe(ov2_btracker *t, int n_active, const ov2_stereo_keyframe_params *params, const ov2_pyr *right,
                                  const uint8_t *do_h, ov2_stereo_keyframe_result *results, float *right_px_h,
                                  uint8_t *stereo_ok_h, uint8_t *tri_status_h, double *wpt_h, double *invdepth_h);
int  ov2_btracker_get_keyframe_info(ov2_btracker *t, int item, int from_device, int *kf_id, double *kf_time, int *kf_nb3dkps,
                                    int *has_info);

/* Mapper::triangulateTemporal on the resident keyframe (f23): what Mapper::run executes on every new keyframe (src/mapper.cpp:107-127;
 * the function is :191-343) for the items ov2_btracker_create_keyframe just turned into keyframes -- in stereo behind
 * ov2_btracker_stereo_keyframe, in mono as the only source of 3-D points -- in ONE enqueue on the context's stream and ONE
 * synchronisation, byte-equal to the route of separate calls (ov2_btracker_get_frame, a walk over the caller's map for src / src_unpx /
 * src_bv and the source poses, ov2_triangulate_keyframe_batch, ov2_btracker_update_frame_batch, ov2_btracker_set_keyframe,
 * ov2_btracker_set_keyframe_info).
 * THE ANCHOR TABLE.  The reference asks its map for the first observing keyframe of a 2-D keypoint (*co_kf_ids.begin(), :262), that
 * keyframe's keypoint (:292) and pose (:278, :332).  A keypoint that has left the current frame can never again be a 2-D keypoint of a
 * new keyframe, so the tracker keeps that record only for the keypoints of the item's latest keyframe: per item at most cfg.n_max
 * records {lmid, row, unpx, bv} ascending by lmid, and at most n_src_max rows {kfid, Twc, Tcw} ascending by kfid, one per keyframe
 * some record still refers to.  The block is allocated by the first call that needs it (ov2_btracker_reserve_anchors, or the first
 * ov2_btracker_temporal_keyframe with its params->n_src_max); another n_src_max afterwards is OV2_EINVAL.
 *   ov2_btracker_set_anchors       installs an item's whole table, as ov2_btracker_set_keyframe installs a keyframe: n records (lmid
 *                                  strictly ascending, kfid[i] the anchoring keyframe, its unpx (2 float) and bv (3 double)) and
 *                                  n_rows rows (row_kfid strictly ascending, row_Twc 7 double each; Tcw = fe_invert_hd(Twc), the
 *                                  arithmetic of ov2_btracker_set_keyframe).  OV2_EINVAL and the state untouched: no block reserved,
 *                                  n outside [0, cfg.n_max], n_rows outside [0, n_src_max], a NULL array, lmid or row_kfid not
 *                                  strictly ascending, a kfid[i] not among the rows, a pose or bv that is not finite, an open call.
 *   ov2_btracker_get_anchors       the table of an item (from_device != 0: copied down, one synchronisation; else the host mirror);
 *                                  arrays of cfg.n_max records / n_src_max rows, any output pointer may be NULL.
 *   ov2_btracker_set_anchor_poses[_batch]   (item, kfid, Twc) triples, the poses local BA moved: ONE upload and ONE launch
 *                                  (k_tkf_set_poses) for the batch, Tcw = fe_invert_hd(Twc).  A kfid that anchors nothing in its item
 *                                  is counted in *n_ignored and ignored.  OV2_EINVAL: an item out of range, a pose not finite, the
 *                                  same (item, kfid) twice, more triples than batch x n_src_max, no block, an open call.
 * THE CALL.  Per item b of [0, n_active) with do_h[b] != 0 whose resident frame is its resident keyframe (csrc/temporalkf.hip):
 *   anchors    k_tkf_anchor: the item's next table, written into its OTHER buffer.  A keypoint of the resident keyframe whose lmid
 *              the current table holds inherits that record; any other is new and anchors at this keyframe (kf_id of the resident
 *              keyframe info) with the kf_unpx / kf_bv k_ckf_install wrote.  Rows that lose their last record go, the others keep their
 *              order, this keyframe's row (Twc / Tcw of the keyframe header) is appended.  More than n_src_max rows:
 *              OV2_TKF_SRC_OVERFLOW, and frame, keyframe and anchors stay what they were.  A table whose newest row is this
 *              keyframe already (a second call on the same keyframe, or ov2_btracker_set_anchors) is taken as it is.
 *   input      k_tkf_input: a slot of the resident frame is a candidate when the keyframe holds its lmid (the reference's
 *              getKeypoints2d() of the keyframe), it is not 3-D (:250) and its anchor is another keyframe than this one (:258-266);
 *              unpx / bv from the keyframe's arrays, src_unpx / src_bv from the anchor.  plm == nullptr (:244) and pkf == nullptr
 *              (:271) CANNOT OCCUR here: the caller removes such observations with ov2_btracker_update_frame and, after its map
 *              culled a keyframe, installs the re-anchored table with ov2_btracker_set_anchors.
 *   triangulation   k_triangulate on the row table with is_stereo = 0 everywhere: the temporal pass alone; params->tri.stereo is
 *              read for the no-motion skip (:287), the left camera's K from params->tri.
 *   apply      k_tkf_apply: every OV2_TRI_TEMPORAL_OK slot gets is3d = 1 and wpt, written into the item's OTHER frame buffer;
 *              kf_nb3dkps of the resident keyframe info is recounted; every OV2_TRI_REMOVE_OBS slot is taken out of the resident
 *              KEYFRAME (removeMapPointObs(lmid, frame.kfid_): the keyframe is compacted in order and its n_kf lowered), not out
 *              of the frame, and the anchor table keeps its record: the first observer has not changed.  _end brings every host
 *              mirror (frame, info, keyframe, anchors) to the same state from what comes down anyway.
 * ONE DEVIATION: if a caller does not run this call for a keyframe it created, the points first seen there anchor at the next
 * keyframe for which it does.
 * results[b].action:
 *   OV2_TKF_NOT_REQUESTED   do_h[b] == 0: nothing of the item is read or written
 *   OV2_TKF_NOT_KEYFRAME    the byte and the rules of OV2_SKF_NOT_KEYFRAME; ov2_btracker_stereo_keyframe does not clear the byte
 *   OV2_TKF_SRC_OVERFLOW    more than n_src_max rows are still referred to: nothing is written
 *   OV2_TKF_DONE            the record and, in the slot space of the resident frame ([0, n) written), tri_status_h (OV2_TRI_* bits),
 *                           wpt_h (3 double), invdepth_h and src_kfid_h (the anchoring keyframe of a candidate, else -1): what a
 *                           caller needs to replay updateMapPoint and removeMapPointObs, and Mapper::run's mono reset test (:129-143)
 * ov2_btracker_last_slot_bytes reports 0 after this call.  OV2_EINVAL, checked on the host before anything is enqueued (the tracker
 * stays where it was): a NULL tracker / params / do_h; n_active outside [1, batch]; an open step, create_keyframe, stereo_keyframe
 * call or call of this kind; no resident block; cfg.n_max > OV2_FKF_MAX_POINTS; n_src_max outside [1, OV2_TKF_MAX_ROWS] or another
 * one than the block's; a non-finite params->tri.K; an item whose table holds a keyframe newer than its resident keyframe.  _end:
 * no open call, a NULL result or output array.  Between _begin and _end the calls that change resident state or start a step
 * return OV2_EINVAL. */
#define OV2_TKF_MAX_ROWS      256
#define OV2_TKF_NOT_REQUESTED 0
#define OV2_TKF_NOT_KEYFRAME  1
#define OV2_TKF_DONE          2
#define OV2_TKF_SRC_OVERFLOW  3
typedef struct {
    ov2_tri_params tri;               /* ov2_triangulate_keyframe_batch: its params, as they are                             */
    int n_src_max;                    /* rows of an item's anchor table: the keyframes its keypoints may anchor at            */
} ov2_temporal_keyframe_params;
typedef struct {
    int action;                       /* OV2_TKF_*; the other fields are 0 unless OV2_TKF_DONE                               */
    int n;                            /* the frame's size                                                                    */
    int n_candidates, n_temporal_good;   /* ov2_tri_result: candidates / good of triangulateTemporal                         */
    int n_remove_obs;                 /* OV2_TRI_REMOVE_OBS slots: keypoints taken out of the keyframe                       */
    int n_no_motion;                  /* OV2_TRI_NO_MOTION slots                                                             */
    int nb3dkps;                      /* is3d slots of the frame after the call: the keyframe info's kf_nb3dkps              */
    int n_rows;                       /* rows of the item's anchor table after the call                                      */
} ov2_temporal_keyframe_result;
int  ov2_btracker_reserve_anchors(ov2_btracker *t, int n_src_max);
int  ov2_btracker_set_anchors(ov2_btracker *t, int item, int n, const int *lmid, const int *kfid, const float *unpx, const double *bv,
                              int n_rows, const int *row_kfid, const double *row_Twc);
int  ov2_btracker_get_anchors(ov2_btracker *t, int item, int from_device, int *n, int *lmid, int *kfid, float *unpx, double *bv,
                              int *n_rows, int *row_kfid, double *row_Twc, double *row_Tcw);
int  ov2_btracker_set_anchor_poses_batch(ov2_btracker *t, int n, const int *item, const int *kfid, const double *Twc, int *n_ignored);
int  ov2_btracker_set_anchor_poses(ov2_btracker *t, int item, int n, const int *kfid, const double *Twc, int *n_ignored);
int  ov2_btracker_temporal_keyframe_begin(ov2_btracker *t, int n_active, const ov2_temporal_keyframe_params *params,
                                          const uint8_t *do_h);
int  ov2_btracker_temporal_keyframe_end(ov2_btracker *t, ov2_temporal_keyframe_result *results, uint8_t *tri_status_h, double *wpt_h,
                                        double *invdepth_h, int *src_kfid_h);
int  ov2_btracker_temporal_keyframe(ov2_btracker *t, int n_active, const ov2_temporal_keyframe_params *params, const uint8_t *do_h,
                                    ov2_temporal_keyframe_result *results, uint8_t *tri_status_h, double *wpt_h, double *invdepth_h,
                                    int *src_kfid_h);

/* ---- the lock-step step from the keyframe: VisualFrontEnd::kltTrackingFromKF (src/visual_front_end.cpp:278-442) -----------------
 * With btrack_keyframetoframe the reference tracks every frame from the LAST KEYFRAME: the template pyramid is kf_pyr_, a copy of
 * the current pyramid taken when the keyframe was created (:52-54), and the source point of a keypoint is the keyframe's px_ of
 * its lmid_ (:336, :346).  ov2_btracker_set_track_from_keyframe(t, 1) puts the step forms that carry lmid --
 * ov2_btracker_track_frame_epi_pose, ov2_btracker_track_mono, ov2_btracker_track_mono_resident -- into that mode; everything behind
 * the tracking stage (computeKeypoint, the filter, the pose chain, the mono tail, the resident frame) runs as before.  It differs
 * from kltTracking in what changes bits:
 *   source      the keyframe's pyramid (the tracker's KEYFRAME STORE: one more pyramid set of `batch` items outside the rotation) and
 *               the keyframe's px of the slot's lmid (the KEYFRAME-PX TABLE: per item [lmid ascending][px], a snapshot taken when the
 *               keyframe was created and only ever looked up by lmid)
 *   membership  a slot whose lmid the item's resident keyframe (ov2_btracker_set_keyframe / _create_keyframe, compacted by
 *               ov2_btracker_temporal_keyframe) no longer holds, or the px table never held, is not tracked: status 4 (bit 2, "not
 *               in the keyframe"), out_xy = its input px.  Every stage behind tests bit 0 or (status & 3) == 1 and treats it as a
 *               lost track, which is what the reference does with it (:316-320, :348-351); it takes no part in the 33 % rule
 *   priors      a slot without a 3-D prior starts from the frame's own px (:343-345), not from its source point
 *   retry       a 3-D-prior slot the one-level pass lost is retried on the full pyramid from the frame's own px (:386), not from
 *               the first pass's forward result; status bit 1 as before
 *   33 % rule   counted over the slots that entered the prior pass.  When it fires, `vpriors = vkps` (:395-400) resets every prior
 *               of the second call: each slot whose result comes from that call (no prior, or bit 1 set) is run again from the
 *               keyframe's item on the full pyramid with prior = the keyframe's px; good prior-pass tracks are kept.  p3p_req and
 *               the re-run of the chains behind follow as in the other mode
 * ov2_btracker_last_priors returns the flag byte the join left: bit 0 the slot entered the prior pass, bit 1 (value 2) it was
 * skipped.
 *
 * ov2_btracker_set_track_from_keyframe   between steps only.  The first `on` allocates the store (OV2_ENOMEM leaves the tracker as it
 *     was, mode off).  While on: the step forms without lmid (ov2_btracker_track_frame, _map, _pose) return OV2_EINVAL; a step in
 *     which an active item carries keypoints but has no adopted keyframe pyramid returns OV2_EINVAL before anything is enqueued (the
 *     reference's `pkf == nullptr` return); ov2_btracker_create_keyframe (both forms) adopts the current pyramid item and installs the
 *     px table of every OV2_CKF_CREATED item in its own enqueue.  While off every call enqueues exactly what it did before; the store
 *     and its contents stay, but an item whose keyframe is replaced while the mode is off (ov2_btracker_create_keyframe creates it,
 *     or ov2_btracker_set_keyframe sets it) loses its adopted pyramid: the store's belongs to the keyframe before, and a step with the
 *     mode on again refuses the item until a pyramid is adopted.  With the mode on, ov2_btracker_set_keyframe leaves the adoption as it
 *     is: the caller that builds keyframes on the host follows it with ov2_btracker_set_keyframe_px and
 *     ov2_btracker_adopt_keyframe_pyramid.
 * The calls below need the store (OV2_EINVAL before the first `on`) and run between steps only:
 * ov2_btracker_adopt_keyframe_pyramid    the current pyramid item of every item b < n_active with do_h[b] != 0 becomes its keyframe
 *     pyramid (one copy kernel, one synchronisation): for callers that build keyframes on the host
 * ov2_btracker_set_keyframe_px           the px table of one item: n <= cfg.n_max entries, lmid strictly ascending, px finite
 * ov2_btracker_get_keyframe_px           the table back, from the host mirror or (from_device != 0) from the device
 * ov2_btracker_kf_item                   item `item` of the store as a batch-1 view (owned by the tracker; NULL without a store)     */
int  ov2_btracker_set_track_from_keyframe(ov2_btracker *t, int on);
int  ov2_btracker_adopt_keyframe_pyramid(ov2_btracker *t, int n_active, const uint8_t *do_h);
int  ov2_btracker_set_keyframe_px(ov2_btracker *t, int item, int n, const int *lmid, const float *px);
int  ov2_btracker_get_keyframe_px(ov2_btracker *t, int item, int from_device, int *n, int *lmid, float *px);
const ov2_pyr *ov2_btracker_kf_item(const ov2_btracker *t, int item);

/* ---- mono initialisation on the resident frame and keyframe (f25): trackMono's un-initialised branch, :98-113 ----------------------
 * ov2_mono_init (above) on the state an ov2_btracker keeps on the device, for the items b < n_active with do_h[b] != 0, in ONE enqueue
 * and ONE synchronisation, without a per-slot byte going up (ov2_btracker_last_slot_bytes gives 0).  It runs right after the
 * ov2_btracker_track_mono_resident step of an item that has not been initialised yet: such an item passes through that step
 * harmlessly (no 3-D keypoints: computePose gives OV2_POSE_TOO_FEW, the filter does not refine, the 33 % rule counts nothing) and its
 * caller ignores the step's keyframe decision.
 *   input    by kernels: lmid / is3d / px of the resident frame's slots in slot order, unpx / bv from px with the tracker's calibration
 *            (k_compute_keypoints: Frame::computeKeypoint), cur_Twc the resident pose, kf_lmid / kf_unpx / kf_bv / kf_Tcw the resident
 *            keyframe (ov2_btracker_set_keyframe, ov2_btracker_create_keyframe); seed_h[b] is the item's seed.
 *   chain    that of ov2_mono_init_batch on a block of the tracker's at capacity; the record of a requested item equals, bit for bit,
 *            what ov2_mono_init returns for those inputs.  removed_h holds cfg.n_max bytes per item, item b's at b * cfg.n_max (the
 *            record's `removed` points there; pair_cur and trace_samples are NULL).
 *   apply    OV2_MINIT_READY: the removed slots leave the resident frame by the rule of OV2_RES_REMOVE (the rest close up in slot
 *            order; the frame is then no longer its keyframe's), and the resident pose becomes Twc_init -- the pose of the UNREFINED
 *            model, see ov2_mono_init.  Any other action leaves frame and pose alone.  EVERY requested item that ran, whatever its
 *            action: the resident motion state becomes MotionModel::reset()'s (prev_time = -1, log_relT = 0, prevTwc stays).  The
 *            reference never reaches updateMotionModel before initialisation (:107 and :111 return first), while the step that ran
 *            for this item did update the state; without the reset the next step would resync and then store a velocity where the
 *            reference stores none.  _end brings the host mirrors (frame, pose, motion) to the same state.
 *   OV2_MINIT_NOT_REQUESTED   do_h[b] == 0: nothing of the item is read or written.
 *   OV2_MINIT_NO_KEYFRAME     the item has no resident keyframe (or an empty one) or no keyframe info (ov2_btracker_set_keyframe_info,
 *                             ov2_btracker_create_keyframe): the reference's pkf == nullptr return (:866); nothing changes.
 * OV2_EINVAL before anything is enqueued, the tracker staying where it was: NULL arguments, n_active outside [1, batch], any open
 * call, no resident frame (ov2_btracker_set_frame), no calibration, cfg.n_max outside [1, OV2_FKF_MAX_POINTS], more than 65535 items,
 * and what ov2_mono_init refuses in its params.  Between _begin and _end the calls that change resident state or start a step return
 * OV2_EINVAL.  The kernels are launched over the items up to the last one that runs.  A HIP error while enqueueing (OV2_EHIP) closes
 * the call; the host mirrors have not moved then, but if the failure came behind the apply kernel the device already holds the new
 * pose and motion state of the requested items: re-install them (ov2_btracker_set_pose, ov2_btracker_reset_motion) or drop the tracker. */
int  ov2_btracker_mono_init_begin(ov2_btracker *t, int n_active, const ov2_mono_init_params *params, const uint8_t *do_h,
                                  const unsigned long long *seed_h);
int  ov2_btracker_mono_init_end(ov2_btracker *t, ov2_mono_init_result *results, uint8_t *removed_h);
int  ov2_btracker_mono_init(ov2_btracker *t, int n_active, const ov2_mono_init_params *params, const uint8_t *do_h,
                            const unsigned long long *seed_h, ov2_mono_init_result *results, uint8_t *removed_h);

#ifdef __cplusplus
}
#endif
#endif /* OV2SLAM_HIP_H */
