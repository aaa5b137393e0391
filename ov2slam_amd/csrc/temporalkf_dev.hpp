// temporalkf_dev.hpp -- what trackb.hip and temporalkf.hip share for ov2_btracker_temporal_keyframe (f23), the lock-step form of
// Mapper::triangulateTemporal on the resident keyframe: the device view of the anchor table (trackb_layout.hpp: BtTkfLayout), the
// device pointers of one call and the launchers.  Between k_tkf_input and k_tkf_apply trackb.hip puts the launch of triangulate.hip
// (k_triangulate on the row table: the temporal pass alone).
//   k_tkf_anchor     in front: the item's next anchor table from the resident keyframe and its current table, the source rows
//   k_tkf_input      the resident frame joined against the keyframe and the anchors into the ranges k_triangulate reads
//   k_tkf_apply      behind k_triangulate: the frame with the new points into the item's other buffer, the keyframe without the
//                    OV2_TRI_REMOVE_OBS keypoints, the record, kf_nb3dkps
//   k_tkf_set_poses  ov2_btracker_set_anchor_poses: the rows of the tables that local BA moved
#pragma once
#include "common.hpp"
#include "frameepi_dev.hpp"
#include "mono_dev.hpp"
#include "resident_dev.hpp"

#define TKF_THREADS 256
#define TKF_WAVES (TKF_THREADS / 64)

// the anchor block: two buffers of `batch` items; item b of buffer s starts at base + s * buf_bytes + b * a_item
struct TkfAnchors {
    uint8_t *base; size_t buf_bytes, a_item, a_lm, a_row, a_un, a_bv, a_nr, a_kf, a_Twc, a_Tcw;
    const uint8_t *sel;                                 // per item: the buffer that holds its current table (0 / 1)
    int n_max, n_src_max;
};

struct TkfItem { int *n, *lmid, *row; float2 *unpx; double *bv; int *n_rows, *kfid; double *Twc, *Tcw; };
__device__ __forceinline__ TkfItem tkf_item(const TkfAnchors &f, int b, int other)
{
    uint8_t *p = f.base + (size_t)(((f.sel[b] != 0) ? 1 : 0) ^ other) * f.buf_bytes + (size_t)b * f.a_item;
    TkfItem it;
    it.n = (int *)p; it.lmid = (int *)(p + f.a_lm); it.row = (int *)(p + f.a_row); it.unpx = (float2 *)(p + f.a_un);
    it.bv = (double *)(p + f.a_bv); it.n_rows = (int *)(p + f.a_nr); it.kfid = (int *)(p + f.a_kf); it.Twc = (double *)(p + f.a_Twc);
    it.Tcw = (double *)(p + f.a_Tcw);
    return it;
}

struct TkfArgs {
    ResFrames f;
    TkfAnchors anc;
    const uint8_t *act;                                 // per item: 1 = asked and the frame is its keyframe
    FeKfHdr *hdr; MonoKfInfo *r_ki;                     // the resident keyframe: its header (n_kf is lowered), its info
    int *kf_lmid; float2 *kf_unpx; double *kf_bv;       // ... and its arrays, n_max slots per item (compacted)
    int n_max;
    // per item, written by k_tkf_anchor / k_tkf_input (trackb_layout.hpp: BtTkfLayout)
    int4 *tit; double *Twc; int *ovf; double *srcT;
    // per slot, n_max slots per item
    float2 *unpx; double *bv; float2 *src_unpx; double *src_bv; int *src; uint8_t *is_stereo;
    // what comes down
    int *src_kfid; const uint8_t *tri_status; const double *tri_wpt;
    ov2_temporal_keyframe_result *rec;
};

int ov2_launch_tkf_anchor(hipStream_t s, const TkfArgs &a, int n_active);
int ov2_launch_tkf_input(hipStream_t s, const TkfArgs &a, int n_active);
int ov2_launch_tkf_apply(hipStream_t s, const TkfArgs &a, int n_active);
int ov2_launch_tkf_set_poses(hipStream_t s, const TkfAnchors &anc, int batch, int n, const int *item_d, const int *kfid_d, const double *Twc_d);
