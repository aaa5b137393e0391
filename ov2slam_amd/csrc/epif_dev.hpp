// epif_dev.hpp -- epipolar2d2dFiltering's chain (epifilter.hip: k_epif_gather, the search of fivept_dev.hpp, k_epif_decide) as host
// steps on a device block the caller owns, so that the lock-step tracker can later put it between k_pose_select and k_pose_pack on
// one stream without a host round trip.  ov2_epipolar_filter_batch is the same launches around one upload, one download and one
// synchronisation, on a block packed to the items' real sizes.
#pragma once
#include "common.hpp"
#include "fivept_dev.hpp"

// 208 bytes.  cur0 / kf0 / row0: where the item's keypoint slots, keyframe slots and sample rows start in the block's arrays (the
// chain's own per-match arrays use the current frame's slots: a frame has at most n_cur matches)
struct EpifItem {
    int cur0, n_cur, kf0, n_kf;
    int row0, n_rows, nb3dkps, nbkfs;
    unsigned long long seed;
    double cur_Twc[7], kf_Tcw[7], kf_Twc[7];
};
static_assert(sizeof(EpifItem) == 208, "EpifItem layout");
struct EpifOut {
    double model[12], F[9], Twc_model[7], score;
    float parallax;
    int action, m, epifrom3dkps, do_optimize, nb3dkps, status, best_row, iterations, rows_consumed, n_inliers, n_outliers;
    int n_removed_ransac, n_removed_sampson, pose_from_model, searched, pad[2];
};
static_assert(sizeof(EpifOut) == 304, "EpifOut layout");

// Offsets from the block's base, every section 16-byte aligned.  [0, o_up): the chain's INPUTS (items, cur_lmid 4, cur_unpx 8,
// cur_bv 24, cur_is3d 1 per current slot; kf_lmid 4, kf_unpx 8, kf_bv 24 per keyframe slot).  [o_up, o_down): its own (bv1 24, bv2 24,
// outliers 4 per current slot; E5Item, E5Out per item; models 96, valid 1, score 8 per row).  [o_down, total): its RESULTS (EpifOut
// per item; removed 1, pair_cur 4, err 4 per current slot; samples 32 per row).
struct EpifLayout {
    size_t B, NC, NK, NR;        // items, current slots, keyframe slots, sample rows
    int s_max;                   // the largest n_rows
    size_t o_it, o_lm, o_un, o_bv, o_3d, o_kl, o_ku, o_kb, o_up;
    size_t o_b1, o_b2, o_ol, o_e5, o_eo, o_md, o_va, o_sc, o_down;
    size_t o_out, o_rm, o_pc, o_er, o_sm, total;
};

// the layout of a block with NC / NK / NR slots in all (the packed form: the sums over the items)
void epif_layout(size_t n_items, size_t NC, size_t NK, size_t NR, int s_max, EpifLayout *L);
// The CAPACITY form, for a block whose items are written on the device: item b owns n_max current and keyframe slots at b * n_max and
// n_rows rows at b * n_rows.  OV2_EINVAL beyond the capacity of ov2_epipolar_filter_batch.
int epif_layout_capacity(int n_items, int n_max, int n_rows, EpifLayout *L);
// what ov2_epipolar_filter_batch checks in its params
int epif_check_params(const ov2_epifilter_params *params);
// The chain on items [0, n_items) of the block `ds`: the gather (join, parallax, gate, packed bearings, E5Item, sample table), the
// three launches of the search, the decision.  No synchronisation; the results are left at [o_down, total).
int epif_chain_enqueue(hipStream_t s, const ov2_epifilter_params *params, const EpifLayout &L, uint8_t *ds, int n_items);
