// mono_dev.hpp -- what trackb.hip and mono.hip share for ov2_btracker_track_mono, the lock-step step that is trackMono after
// initialisation: the motion model in front of the step of f18 / f16, and behind it the frame checkNewKfReq sees, the model's update
// and the keyframe decision.  The device pointers of a step, and the two launchers.
#pragma once
#include "common.hpp"
#include "fkf_dev.hpp"
#include "pose_dev.hpp"
#include "frameepi_dev.hpp"

// 16 bytes per item, device resident: ov2_btracker_set_keyframe_info
struct MonoKfInfo { int kf_id, kf_nb3dkps, has_info, pad; };
static_assert(sizeof(MonoKfInfo) == 16, "MonoKfInfo layout");

struct MonoArgs {
    // resident (trackb_layout.hpp: the resident block; the keyframe headers of the epipolar side)
    double *r_T; ov2_motion_state *r_st; const double *r_kt; const MonoKfInfo *r_ki; const FeKfHdr *hdr;
    // the step's inputs: one per item
    const double *time; const int *frame_id, *localba;
    // k_mono_apply: the predicted pose into the pose block (q_T) and the result block (pT), its inverse into the map block (m_T), the
    // state after the resync (sa), resynced
    double *q_T, *m_T, *pT; ov2_motion_state *sa; uint8_t *rs;
    // k_mono_pack reads the tracker's blocks (n_max slots per item) and the step's results in slot space; epi_removed: NULL without the
    // filter; pose_out: NULL when no chain ran (a step with no keypoint anywhere: every frame is empty, the pose is the predicted one)
    const int *n_dev; const uint8_t *status, *is3d; const float2 *out_xy, *unpx; const double *bv; const int *lmid;
    const uint8_t *epi_removed, *pose_removed; const PoseOut *pose_out;
    // ... and writes the packed frame, the item records, the count, the state after the update (su; and the resident pose and state)
    FkfItemD *items; int *c_lmid; float2 *c_px, *c_unpx; double *c_bv; uint8_t *c_is3d; int *ncur_io; ov2_motion_state *su;
    int n_max;
};

int ov2_launch_mono_apply(hipStream_t s, const MonoArgs &a, int n_active);
int ov2_launch_mono_pack(hipStream_t s, const MonoArgs &a, int n_active);
