// resident_dev.hpp -- what trackb.hip and resident.hip share for the resident frame (f21): the current frame of every item of an
// ov2_btracker kept on the device from step to step (trackb_layout.hpp: BtResLayout).  The device view of the frame block, the
// pointers of the five launches, the per-item functions of the kernels, and the launchers.
//   k_res_update   ov2_btracker_update_frame: what the map did to a frame (SET_POINT / UNSET_POINT / REMOVE by lmid)
//   k_res_stage    in front of a resident step: the frame into the locations the step's kernels read
//   k_res_carry    behind k_mono_pack: the frame the step leaves, by k_mono_pack's own rule, as the item's next resident frame
//   k_res_ckf_in   in front of a resident create_keyframe: the frame into that call's input ranges
//   k_res_adopt    behind k_ckf_install: the frame with the new points appended becomes the resident frame of a CREATED item
#pragma once
#include "common.hpp"
#include "pose_dev.hpp"

#define RES_THREADS 256
#define RES_WAVES (RES_THREADS / 64)

// the frame block: two buffers of `batch` items; item b of buffer s starts at base + s * buf_bytes + b * f_item
struct ResFrames {
    uint8_t *base; size_t buf_bytes, f_item, f_px, f_lm, f_3d, f_w;
    const uint8_t *sel;                                 // per item: the buffer that holds its current frame (0 / 1)
    int n_max;
};

struct ResItem { int *n; float2 *px; int *lmid; uint8_t *is3d; double *wpt; };
__device__ __forceinline__ ResItem res_item(const ResFrames &f, int b, int other)
{
    uint8_t *p = f.base + (size_t)(((f.sel[b] != 0) ? 1 : 0) ^ other) * f.buf_bytes + (size_t)b * f.f_item;
    ResItem it;
    it.n = (int *)p; it.px = (float2 *)(p + f.f_px); it.lmid = (int *)(p + f.f_lm); it.is3d = p + f.f_3d; it.wpt = (double *)(p + f.f_w);
    return it;
}
__device__ __forceinline__ int res_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// k_mono_pack's rule (mono.hip), restated: the slot is tracked and was removed neither by the filter (epi_removed NULL: the filter
// did not run) nor by the pose
__device__ __forceinline__ bool res_keep(const uint8_t *status, const uint8_t *epi_removed, const uint8_t *pose_removed, size_t s)
{
    return (status[s] & 3) == 1 && !(epi_removed && epi_removed[s] != 0) && pose_removed[s] == 0;
}
// ... and the number of slots it looks at: none where computePose reset the frame (resetFrame()) or where no chain ran
__device__ __forceinline__ int res_keep_count(const PoseOut *pose_out, const int *n_dev, int b, int n_max)
{
    if (!pose_out) return 0;
    const int action = pose_out[b].action;
    return (action == OV2_POSE_P3P_RESET || action == OV2_POSE_PNP_RESET) ? 0 : res_clamp(n_dev[b], n_max);
}

// Compaction in slot order, the scheme of k_mono_pack: one round of RES_THREADS slots; `keep` is this thread's slot.  Returns the
// slot's rank among the kept ones of the item so far (valid where keep) and advances `m` by the round's count.  s_w: two sets of
// per-wavefront counts, so one barrier a round.
__device__ __forceinline__ int res_rank(bool keep, int round, int (*s_w)[RES_WAVES], int &m)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long mk = __ballot(keep);
    int *sw = s_w[round & 1];
    if (lane == 0) sw[wave] = __popcll(mk);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < RES_WAVES; w++) { const int c = sw[w]; all += c; before += w < wave ? c : 0; }
    const int r = m + before + __popcll(mk & ((1ull << lane) - 1ull));
    m += all;
    return r;
}

// ov2_btracker_update_frame: the op lists, packed (item b's n_ops[b] ops start at ops[op_off[b]]), and the records
struct ResUpdateArgs {
    ResFrames f;
    const int *n_ops, *op_off; const ov2_resident_op *ops;
    ov2_resident_update_result *rec;
};

// a resident step: where stage_points / stage_map / stage_epi / stage_pose put the per-slot inputs (n_max slots per item) ...
struct ResStageArgs {
    ResFrames f;
    float2 *kps; double *wpt; uint8_t *is3d; int *lmid; int *scale;
};
// ... and what k_mono_pack reads, for the frame the step leaves
struct ResCarryArgs {
    ResFrames f;
    const int *n_dev; const uint8_t *status, *epi_removed, *pose_removed; const PoseOut *pose_out;
    const float2 *out_xy; const int *lmid; const uint8_t *is3d; const double *wpt;
};

// ov2_btracker_create_keyframe on the resident frame: the call's input ranges, and after k_ckf_install its frame and records
struct ResCkfArgs {
    ResFrames f;
    const uint8_t *flag; int *n; float2 *px; int *lmid; uint8_t *is3d;
    const ov2_create_keyframe_result *rec;
};

int ov2_launch_res_update(hipStream_t s, const ResUpdateArgs &a, int item0, int n_items, int ops_cap);   // items [item0, item0 + n_items)
int ov2_launch_res_stage(hipStream_t s, const ResStageArgs &a, int n_active);
int ov2_launch_res_carry(hipStream_t s, const ResCarryArgs &a, int n_active);
int ov2_launch_res_ckf_in(hipStream_t s, const ResCkfArgs &a, int n_active);
int ov2_launch_res_adopt(hipStream_t s, const ResCkfArgs &a, int n_active);
