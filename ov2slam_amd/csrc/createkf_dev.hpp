// createkf_dev.hpp -- what trackb.hip and createkf.hip share for ov2_btracker_create_keyframe, the lock-step form of
// MapManager::createKeyframe: the device pointers of one call and the three launchers.  Between them trackb.hip puts the launches
// of detect.hip (enqueue_detect), keypoint.hip (k_compute_keypoints) and brief.hip (k_brief32).
#pragma once
#include "common.hpp"
#include "frameepi_dev.hpp"
#include "mono_dev.hpp"

struct CkfArgs {
    // per item, from the host (trackb_layout.hpp: BtCkfLayout): the frame's size, the request, nlmid_, the keyframe's id and time, its
    // pose (the call's, or the resident one of ov2_btracker_track_mono)
    const int *n; const uint8_t *flag; const int *nlmid, *nkfid; const double *time, *Twc;
    // the frame, n_max slots per item: in with n[b] keypoints, out with the new ones appended
    float2 *px; int *lmid; const uint8_t *is3d;
    // the detector's side: its skip byte and, behind it, its counts (the int at so_n[b * so_stride]) and points (det_cap per item)
    uint8_t *skip; const int *so_n; int so_stride; const float2 *det; int det_cap;
    int *nb;                                            // the frame's size where computeKeypoint and BRIEF run, else 0
    // level 0 of the current pyramid (the colour of a new point)
    const uint8_t *img; long long img_item; int img_pitch, w, h;
    // results: the record, colour per new slot, and for the host mirrors the header and the slot of the keyframe's i-th id
    ov2_create_keyframe_result *rec; uint8_t *color; FeKfHdr *o_hdr; int *perm;
    const float2 *unpx; const double *bv;               // computeKeypoint's output over the new frame
    // resident: the keyframe arrays and headers of ov2_btracker_set_keyframe, the info of ov2_btracker_set_keyframe_info
    int *kf_lmid; float2 *kf_unpx; double *kf_bv; FeKfHdr *hdr; MonoKfInfo *r_ki; double *r_kt;
    int n_max, ncellsize, nbwcells, nbhcells, nbmaxkps, det_on;
};

int ov2_launch_ckf_prepare(hipStream_t s, const CkfArgs &a, int n_active);   // noccupcells, nb3dkps, nb2detect, the skip byte
int ov2_launch_ckf_append(hipStream_t s, const CkfArgs &a, int n_active);    // addKeypointsToFrame: px, lmid, colour; the overflow
int ov2_launch_ckf_install(hipStream_t s, const CkfArgs &a, int n_active);   // addKeyframe: the sort by lmid, the resident keyframe
