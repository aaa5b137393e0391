// pose_dev.hpp -- computePose's chain (pnp.hip: the search of p3p_dev.hpp, k_pose_gather, k_pnp_solve, k_pose_decide) as host steps
// on a device block the caller owns, so that the lock-step tracker (trackb.hip, framepose.hip) can put the chain behind its own
// kernels on one stream without a host round trip.  ov2_compute_pose_batch is the same launches around one upload, one download and
// one synchronisation, on a block packed to the problems' real sizes.
#pragma once
#include "common.hpp"
#include "p3p_dev.hpp"

struct PnPItem { int n, pt0, pad0, pad1; };
struct PnPOut {
    double pose[7], initial_cost[2], final_cost[2];
    int success, n_out, ran[2], iterations[2], n_success[2], termination[2];
};
static_assert(sizeof(PnPOut) == 128, "PnPOut layout");

struct PoseItem { int n, pt0, do_p3p, p3p_req; };
struct PoseOut {
    double Twc[7], p3p_score, initial_cost[2], final_cost[2];
    int action, p3p_req_out, n_removed_p3p, n_outliers_pnp, ran_p3p, p3p_status, p3p_best_row, p3p_iterations, p3p_rows_consumed;
    int ran[2], iterations[2], n_success[2], termination[2], pad;
};
static_assert(sizeof(PoseOut) == 168, "PoseOut layout");

// The chain's device block in its CAPACITY form: every item owns n_max point slots (pt0 = b * n_max) and n_rows sample rows
// (row0 = b * n_rows); the real counts are the ones the device items hold.  Offsets are from the block's base, every section
// 16-byte aligned.  [items][unpx 16][sigma 8][the search's block: P3Item, bv 24, X 24, samples 16, ...] are the chain's INPUTS (the
// world points are read from the search's X: one copy serves both); the rest is the chain's own.
struct PoseLayout {
    size_t B; int n_max, n_rows;
    P3Plan pl;
    size_t o_it, o_px, o_sg, o_p3, o_cx, o_cw, o_cs, o_ix, o_pi, o_q0, o_st, o_po, o_pl, o_rm, total;
};

// what ov2_compute_pose_batch checks in its params (NULL, the PnP settings, the search's settings)
int pose_check_params(const ov2_pose_params *params);
// OV2_EINVAL beyond the capacity (OV2_P3P_MAX_POINTS / OV2_P3P_MAX_ROWS per item, 65535 items, 2^31 - 1 points or rows in all)
int pose_layout(int n_items, int n_max, int n_rows, PoseLayout *L);
// The chain on items [0, n_items) of the block: the three launches of the search when `search` (some item may have do_p3p), the
// gather, k_pnp_solve, the decision.  Twc_d: 7 doubles per item; out_d: one PoseOut per item; the removal bytes (packed space, item
// b's at b * n_max) are left at o_rm.
int pose_chain_enqueue(hipStream_t s, const ov2_pose_params *params, const PoseLayout &L, uint8_t *ds, const double *Twc_d, PoseOut *out_d,
                       int n_items, bool search);

// framepose.hip: the pose set, computePose's chain and the removal bytes in slot space, behind k_compute_keypoints.  The device
// pointers of a step, named as the kernels' FpArgs names them: the tracker's point block (n_dev, status, unpx, bv) and map block
// (wpt, is3d); the step's pose inputs (Twc, scale, flags, seed) and results (out, ms, removed_slot) in its pinned or mirrored block;
// work: [PoseLayout L][sel 1][slot 4][rank 4 per slot].
struct FramePoseIo {
    const int *n_dev; const uint8_t *status; const float *unpx; const double *bv, *wpt; const uint8_t *is3d;
    const double *Twc; const int *scale; const uint8_t *flags; const unsigned long long *seed;
    uint8_t *work; PoseOut *out; int *ms; uint8_t *removed_slot;
};
// what a step enqueues between the select and the pack (frameepi.hip: ov2_frame_epi_hook, or none): it may clear select bytes
typedef int (*ov2_fp_hook)(hipStream_t s, uint8_t *sel, void *arg);
int ov2_launch_frame_pose(hipStream_t s, const ov2_pose_params *params, const PoseLayout &L, int n_active, bool search, const FramePoseIo &io,
                          ov2_fp_hook hook, void *hook_arg);
// bytes of the work block for layout L, and where the slot list of the packed points lies in it
size_t ov2_frame_pose_work_bytes(const PoseLayout &L);
size_t ov2_frame_pose_slot_offset(const PoseLayout &L);
