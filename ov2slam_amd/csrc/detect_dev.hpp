// detect_dev.hpp -- what detect.hip shares with a caller that enqueues the grid detectors on buffers of its own (trackb.hip: the
// lock-step tracker's createKeyframe, where the detection sits between other kernels of one enqueue and the counts stay on the
// device): the records the kernels exchange, the per-item argument block, and the three launches.
#pragma once
#include "common.hpp"
#include "detect_plan.hpp"

struct CellCand { int p1; float v1; int p2; float v2; };      // p = lx | ly << 16 (cell-local pixel), -1: none
static_assert(sizeof(CellCand) == DET_CAND_BYTES, "detect_plan.hpp lays out the scratch with this size");

// Batched launches (one image per batch item of a pyramid, ov2_detect_*_batch_d): per-item strides and parameters; everything
// zero / NULL for a single image.  The cell kernels run ncells work-groups per item, the selection one work-group per item,
// the sub-pixel refinement a wavefront per (output slot, item).
struct DetBatch {
    long long img_stride;      // bytes between the items' images
    int ncells;                // cells per image
    int cur_stride;            // float2 entries between the items' current-keypoint lists
    int out_stride;            // float2 entries between the items' output lists
    const int *ncur;           // per-item number of current keypoints   (NULL: ncur_all)
    const float2 *cur;         // item 0's current keypoints (the cell kernels skip occupied cells like the reference's loop does)
    int ncur_all;              // number of current keypoints when ncur == NULL
    const int *fast_th;        // per-item FAST threshold                (NULL: the scalar argument)
    const double *quality;     // per-item quality level                 (NULL: SelectParams::quality)
    const uint8_t *skip;       // per-item byte, non-zero: no detection for this item -- its work-groups leave at once, its free-cell
                               // list is empty and its SelectOut is all zero, so the sub-pixel pass leaves too (NULL: every item runs)
};

struct SelectOut {
    int n;               // points written to out_xy
    int nboccup, nbempty, nbkps;
    int nslow, pad_;             // cells of the sweep that needed the full masked scan (a candidate was hit by a neighbour's disc)
    unsigned long long dbg[4];   // wall_clock64 ticks (100 MHz): init, prologue, sweep, compaction
};
static_assert(sizeof(SelectOut) == DET_SELECT_OUT_BYTES, "detect_plan.hpp lays out the scratch with this size");

// what an entry point does before its first enqueue_detect: the geometry check (OV2_EUNSUPPORTED with the detectors' messages) and
// the kernels' dynamic-LDS limits, raised once per process
int det_ready(const ov2_ctx *ctx, int w, int h, int cell, int mode);

// The three launches of a detection (response + candidates per cell, selection, sub-pixel refinement) for `items` images
// that lie `B.img_stride` bytes apart; every pointer addresses item 0.  Asynchronous on `stream`; the context gives the options only.
// mode 0: detectGridFAST, 1: detectSingleScale.  The counts stay on the device (so_d[item].n).
int enqueue_detect(const ov2_ctx *ctx, hipStream_t stream, int mode, const uint8_t *im, int w, int h, int im_stride, int cell, int items, DetBatch B,
                   int fast_th, int mask_mode, const int roi[4], double quality, int ncur, const float2 *cur_d,
                   uint8_t *maps_d, CellCand *cand_d, int *free_d, float2 *out_d, SelectOut *so_d, int do_subpix);
