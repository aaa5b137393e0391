// frameepi_dev.hpp -- what trackb.hip and frameepi.hip share for the lock-step step with epipolar2d2dFiltering between tracking and
// pose (ov2_btracker_track_frame_epi_pose): the resident keyframe header, the kernels' argument block and the hook that
// ov2_launch_frame_pose (framepose.hip) calls between k_pose_select and k_pose_pack.
#pragma once
#include "common.hpp"
#include "epif_dev.hpp"
#include "pose_dev.hpp"

// 120 bytes per item, device resident: written by ov2_btracker_set_keyframe, read by k_epif_pack.  All zero: no keyframe.
struct FeKfHdr {
    int n_kf, pad;
    double kf_Twc[7], kf_Tcw[7];
};
static_assert(sizeof(FeKfHdr) == 120, "FeKfHdr layout");

struct FeArgs {
    // the tracker's blocks: n_max slots per item
    const int *n_dev; const uint8_t *status, *is3d; const float2 *unpx; const double *bv;
    // the step's inputs: lmid per slot; nbkfs, seed, Twc[7] per item; the resident keyframe headers
    const int *lmid, *nbkfs; const unsigned long long *seed; const double *Twc; const FeKfHdr *hdr;
    // the chain's inputs in the epipolar block (EpifLayout at capacity: item b's slots at b * n_max)
    EpifItem *items; int *c_lmid; float2 *c_unpx; double *c_bv; uint8_t *c_is3d;
    int *slot, *rank;                                   // slot of packed keypoint k, packed rank of slot i (-1: not in the frame)
    // the chain's results (packed space) and where they go in slot space: the step's result block, and the select bytes
    const EpifOut *out; const uint8_t *removed; const float *err; const int *pair_cur;
    uint8_t *sel;
    EpifOut *out_io; int *ncur_io; uint8_t *removed_io; float *err_io; int *pair_io;
    int n_max, n_rows;
};

// k_epif_pack, the chain (epif_chain_enqueue), k_epif_apply on `s`; a.sel is set by the caller of the hook
struct FeStep {
    FeArgs a;
    const ov2_epifilter_params *params;
    EpifLayout L;
    uint8_t *block;                                     // the epipolar block
    int n_active;
};
int ov2_frame_epi_hook(hipStream_t s, uint8_t *sel, void *arg);     // an ov2_fp_hook (pose_dev.hpp); arg: FeStep *
// [t q] of the inverse of the transform [t q] (Sophus' SE3::inverse: the conjugate, and minus the rotated translation).  Products,
// sums and negations only, compiled without contraction: host and device (motion.hip) give the same bits.  out may not alias T.
__host__ __device__ inline void fe_invert_hd(const double *T, double *out)
{
    const double x = -T[3], y = -T[4], z = -T[5], w = T[6];        // the conjugate
    const double R[9] = {1. - 2. * (y * y + z * z), 2. * (x * y - z * w), 2. * (x * z + y * w),
                         2. * (x * y + z * w), 1. - 2. * (x * x + z * z), 2. * (y * z - x * w),
                         2. * (x * z - y * w), 2. * (y * z + x * w), 1. - 2. * (x * x + y * y)};
    for (int r = 0; r < 3; r++) out[r] = -((R[3 * r] * T[0] + R[3 * r + 1] * T[1]) + R[3 * r + 2] * T[2]);
    out[3] = x; out[4] = y; out[5] = z; out[6] = w;
}
void ov2_fe_invert(const double T[7], double out[7]);
