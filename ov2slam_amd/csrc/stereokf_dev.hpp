// stereokf_dev.hpp -- what trackb.hip and stereokf.hip share for ov2_btracker_stereo_keyframe (f22), the lock-step form of the
// mapper's stereo block on the resident keyframe (MapManager::stereoMatching, then Mapper::triangulateStereo): the device pointers
// of one call and the four launchers.  Between them trackb.hip puts the launches of priors.hip (k_prior_stereo), stereo.hip
// (k_line_min_sad, k_epipolar_check), lk.hip / lkw.hip (k_track_klt) and triangulate.hip (k_triangulate).
//   k_skf_input      in front: the resident frame and the keyframe header into the ranges those kernels read, unpx / bv of the left
//                    camera, the per-item descriptors, and without rectification the keypoint grid in slot order
//   k_skf_seed       between k_prior_stereo and the tracking: flag = has_prior != 0 and, without rectification, "nothing found"
//   k_skf_stereo_kp  behind k_epipolar_check: stereo_ok, right_px, the right camera's computeKeypoint, is_stereo
//   k_skf_apply      behind k_triangulate: the frame with the new points into the item's other buffer, the record, kf_nb3dkps
#pragma once
#include "common.hpp"
#include "keypoint_dev.hpp"
#include "frameepi_dev.hpp"
#include "mono_dev.hpp"
#include "resident_dev.hpp"

#define SKF_THREADS 256
#define SKF_WAVES (SKF_THREADS / 64)

// priors.hip's PriItemD: first keypoint and count; first entry of the item's cell_start and of its cell_kp
struct SkfItemD { int p0, n, cell0, ck0; };
static_assert(sizeof(SkfItemD) == 16, "SkfItemD layout");

struct SkfArgs {
    ResFrames f;
    const uint8_t *act;                                 // per item: 1 = OV2_SKF_DONE
    const FeKfHdr *hdr; MonoKfInfo *r_ki;               // the resident keyframe: its header, its info
    KpCalib left, right;
    int n_max, rect, nbw, nbh;                          // the grid of Frame::getSurroundingKeypoints (rect: none)
    float cellsize, down;                               // (float)ncellsize; 1 / 2^level: the keypoint on the coarsest level
    // per item, written by k_skf_input (trackb_layout.hpp: BtSkfLayout)
    SkfItemD *pit; int4 *tit; double *Tcw, *Twc; int *nd;
    // per slot, n_max slots per item
    float2 *px, *unpx; double *bv, *fw; float2 *top; uint8_t *state; int *src; int *cell_start, *cell_kp;
    const uint8_t *has_prior; uint8_t *flag; float *sadx;
    const float2 *lk_out; const uint8_t *lk_st, *gate_ok; float2 *runpx; double *rbv; uint8_t *is_stereo;
    // what comes down: the five per-slot outputs and the record
    float2 *right_px; uint8_t *stereo_ok; const uint8_t *tri_status; const double *tri_wpt;
    ov2_stereo_keyframe_result *rec;
};

int ov2_launch_skf_input(hipStream_t s, const SkfArgs &a, int n_active);
int ov2_launch_skf_seed(hipStream_t s, const SkfArgs &a, int n_active);
int ov2_launch_skf_stereo_kp(hipStream_t s, const SkfArgs &a, int n_active);
int ov2_launch_skf_apply(hipStream_t s, const SkfArgs &a, int n_active);
