// monoinit_dev.hpp -- the mono initialisation chain (monoinit.hip: k_fkf_parallax of fkf.hip, k_minit_gather, the search of
// fivept_dev.hpp, k_minit_decide) as host steps on a device block the caller owns, as epif_dev.hpp does for epipolar2d2dFiltering.
// ov2_mono_init_batch is these launches around one upload, one download and one synchronisation, on a block packed to the items'
// real sizes.
#pragma once
#include "common.hpp"
#include "fivept_dev.hpp"
#include "fkf_dev.hpp"
#include "frameepi_dev.hpp"
#include "resident_dev.hpp"

// what the chain needs beside the FkfItemD of the same index (cur0 / n_cur / kf0 / n_kf and the two poses are read from that one; the
// chain's own per-match arrays use the current frame's slots, as in epif_dev.hpp)
struct MinitItem {
    int row0, n_rows;            // where the item's sample rows start, and how many it may draw
    unsigned long long seed;
};
static_assert(sizeof(MinitItem) == 16, "MinitItem layout");
struct MinitOut {
    double model[12], Twc_init[7], score;
    float p0, p1;
    int action, nb2dkps, p0_n, p0_n_distinct, p0_n_nonfinite, m, status, best_row, iterations, rows_consumed, n_inliers, n_outliers;
    int n_removed, searched;
};
static_assert(sizeof(MinitOut) == 224, "MinitOut layout");

// Offsets from the block's base, every section 16-byte aligned.  [0, o_up): the chain's INPUTS (FkfItemD and MinitItem per item;
// cur_lmid 4, cur_unpx 8, cur_bv 24, cur_is3d 1 per current slot; kf_lmid 4, kf_unpx 8, kf_bv 24 per keyframe slot).  [o_up, o_down):
// its own (FKF_OUT_INTS ints, E5Item, E5Out per item; bv1 24, bv2 24, outliers 4 per current slot; models 96, valid 1, score 8 per
// row).  [o_down, total): its RESULTS (MinitOut per item; removed 1, pair_cur 4 per current slot; samples 32 per row).
struct MinitLayout {
    size_t B, NC, NK, NR;        // items, current slots, keyframe slots, sample rows
    int s_max;                   // the largest n_rows
    size_t o_fi, o_mi, o_lm, o_un, o_bv, o_3d, o_kl, o_ku, o_kb, o_up;
    size_t o_fo, o_b1, o_b2, o_ol, o_e5, o_eo, o_md, o_va, o_sc, o_down;
    size_t o_out, o_rm, o_pc, o_sm, total;
};

// the layout of a block with NC / NK / NR slots in all (the packed form: the sums over the items)
void minit_layout(size_t n_items, size_t NC, size_t NK, size_t NR, int s_max, MinitLayout *L);
// The CAPACITY form, for a block whose items are written on the device: item b owns n_max current and keyframe slots at b * n_max and
// n_rows rows at b * n_rows.  OV2_EINVAL beyond the capacity of ov2_mono_init_batch.
int minit_layout_capacity(int n_items, int n_max, int n_rows, MinitLayout *L);
// what ov2_mono_init_batch checks in its params
int minit_check_params(const ov2_mono_init_params *params);
// keyframe arrays that lie outside the block (the lock-step tracker's resident keyframes): item b's at its kf0, as in the block
struct MinitKf { const int *lmid; const float2 *unpx; const double *bv; };
// The chain on items [0, n_items) of the block `ds`: p0 (k_fkf_parallax), the gather (nb2dkps, the gates, the join, p1, packed
// bearings, E5Item, sample table), the three launches of the search, the decision.  kf: where the keyframe arrays lie when not in the
// block's own sections (NULL: there).  No synchronisation; the results are left at [o_down, total).
int minit_chain_enqueue(hipStream_t s, const ov2_mono_init_params *params, const MinitLayout &L, uint8_t *ds, int n_items,
                        const MinitKf *kf = nullptr);
// the record of a result from what the chain left (the three pointers of the result are not touched)
void minit_record(const MinitOut &o, ov2_mono_init_result *r);

// ---- ov2_btracker_mono_init (trackb_monoinit.hip): the chain on the resident frame and keyframe of a lock-step tracker ----------------
//   k_minit_input   in front: one thread per slot of a requested item's resident frame -- lmid, is3d and px into the chain's block and
//                   the range Frame::computeKeypoint reads (ov2_launch_compute_keypoints follows), the FkfItemD (the resident pose, the
//                   keyframe's count and inverse pose) and the MinitItem.  An item that is not requested gets an empty record.
//   k_minit_apply   behind the chain, ONE WORK-GROUP PER REQUESTED ITEM: the record and the removal flags into the range that comes
//                   down; OV2_MINIT_READY: the frame without the removed slots, closed up in slot order, into the item's OTHER buffer
//                   (res_rank: the scheme of k_res_update) and Twc_init as the resident pose; every requested item: the resident
//                   motion state as MotionModel::reset() leaves it.
struct MinitTrackArgs {
    ResFrames f;
    const uint8_t *act;                                 // per item: 1 = requested and it has a resident keyframe with its info
    const unsigned long long *seed;
    double *r_T; ov2_motion_state *r_st;                // the resident pose and motion state
    const FeKfHdr *hdr;                                 // the resident keyframes' headers
    int n_max, n_rows;
    int *nd; float2 *px;                                // device only: the count and the px of every item, n_max slots per item
    FkfItemD *fi; MinitItem *mi; int *cur_lmid; uint8_t *cur_is3d;      // the chain's inputs (its block at capacity)
    const MinitOut *out; const uint8_t *removed;        // ... and its results
    MinitOut *rec; uint8_t *rm;                         // what comes down (trackb_layout.hpp: BtMinitLayout)
};
int ov2_launch_minit_input(hipStream_t s, const MinitTrackArgs &a, int n_active);
int ov2_launch_minit_apply(hipStream_t s, const MinitTrackArgs &a, int n_active);
