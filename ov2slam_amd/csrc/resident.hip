// resident.hip -- the kernels of the resident frame (f21; trackb.hip): the current frame of every item of an ov2_btracker -- per slot
// px, lmid, is3d and the 3-D point -- stays on the device between the lock-step steps, in a block of two buffers per item
// (trackb_layout.hpp: BtResLayout).  A kernel reads an item's frame from its current buffer and writes the next frame into the other
// one, so the frame before a step survives until the step's _end decides which of the two holds.
//   k_res_update   ov2_btracker_update_frame: ONE WORK-GROUP OF FOUR WAVEFRONTS PER ITEM.  The op list's (lmid, op) in LDS; each
//                  thread owns slots tid, tid + 256, ... and scans the list for its own lmid (every lane reads the same entry: a
//                  broadcast); SET_POINT / UNSET_POINT change the slot, REMOVE drops it, the rest close up in slot order.
//   k_res_stage    one thread per slot: the frame into the point, map, epipolar and pose blocks, where the step's kernels read it.
//   k_res_carry    one work-group per item behind k_mono_pack, by its rule (resident_dev.hpp: res_keep): the tracked px of the kept
//                  slots with their lmid, is3d and point, in slot order.
//   k_res_ckf_in   one work-group per flagged item: the frame into the input ranges of ov2_btracker_create_keyframe.
//   k_res_adopt    one work-group per item behind k_ckf_install: where the record says OV2_CKF_CREATED, the call's frame (the old
//                  slots, then the new points with is3d = 0 and a zero point) becomes the item's next resident frame.
// The compaction is k_mono_pack's: a ballot per wavefront, the wavefronts' counts in LDS, one barrier a round.  No atomics, no
// scratch; every count read from device memory is clamped against n_max before it indexes anything.
#include "resident_dev.hpp"

static_assert(sizeof(ov2_resident_op) == 32 && sizeof(ov2_resident_update_result) == 24, "resident records");

__global__ __launch_bounds__(RES_THREADS) void k_res_update(ResUpdateArgs a, int item0, int ops_cap)
{
    __shared__ int s_lm[OV2_FKF_MAX_POINTS];
    __shared__ uint8_t s_op[OV2_FKF_MAX_POINTS];
    __shared__ int s_w[2][RES_WAVES];
    __shared__ int s_tot[RES_WAVES][3];
    const int b = item0 + blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int nm = a.f.n_max < OV2_FKF_MAX_POINTS ? a.f.n_max : OV2_FKF_MAX_POINTS;
    const ResItem src = res_item(a.f, b, 0), dst = res_item(a.f, b, 1);
    const int n = res_clamp(*src.n, nm);
    const int off = res_clamp(a.op_off[b], ops_cap);
    const int nop = res_clamp(a.n_ops[b], nm < ops_cap - off ? nm : ops_cap - off);
    const ov2_resident_op *ops = a.ops + off;
    for (int j = t; j < nop; j += RES_THREADS) { s_lm[j] = ops[j].lmid; s_op[j] = (uint8_t)ops[j].op; }
    __syncthreads();
    int m = 0, c_set = 0, c_unset = 0, c_rem = 0;
    for (int i0 = 0, round = 0; i0 < n; i0 += RES_THREADS, round++) {
        const int i = i0 + t;
        const bool in = i < n;
        int lm = 0, hit = -1; float2 px = make_float2(0.f, 0.f); double w0 = 0., w1 = 0., w2 = 0.; uint8_t d3 = 0;
        if (in) {
            lm = src.lmid[i]; px = src.px[i]; d3 = (uint8_t)(src.is3d[i] != 0); w0 = src.wpt[3 * i]; w1 = src.wpt[3 * i + 1]; w2 = src.wpt[3 * i + 2];
            for (int j = 0; j < nop; j++) hit = s_lm[j] == lm ? j : hit;        // (an id stands once in a list: the host checked)
        }
        const int op = hit >= 0 ? (int)s_op[hit] : -1;
        const bool set = op == OV2_RES_SET_POINT, unset = op == OV2_RES_UNSET_POINT, rem = op == OV2_RES_REMOVE;
        if (set) { w0 = ops[hit].xyz[0]; w1 = ops[hit].xyz[1]; w2 = ops[hit].xyz[2]; d3 = 1; }
        if (unset) d3 = 0;
        c_set += __popcll(__ballot(set)); c_unset += __popcll(__ballot(unset)); c_rem += __popcll(__ballot(rem));
        const bool keep = in && !rem;
        const int r = res_rank(keep, round, s_w, m);                            // r <= i < n_max
        if (keep) { dst.lmid[r] = lm; dst.px[r] = px; dst.is3d[r] = d3; dst.wpt[3 * r] = w0; dst.wpt[3 * r + 1] = w1; dst.wpt[3 * r + 2] = w2; }
    }
    if (lane == 0) { s_tot[wave][0] = c_set; s_tot[wave][1] = c_unset; s_tot[wave][2] = c_rem; }
    __syncthreads();
    if (t != 0) return;
    int n_set = 0, n_unset = 0, n_rem = 0;
#pragma unroll
    for (int w = 0; w < RES_WAVES; w++) { n_set += s_tot[w][0]; n_unset += s_tot[w][1]; n_rem += s_tot[w][2]; }
    *dst.n = m;
    ov2_resident_update_result r;
    r.n_before = n; r.n_after = m; r.n_set = n_set; r.n_unset = n_unset; r.n_removed = n_rem; r.n_missing = nop - (n_set + n_unset + n_rem);
    a.rec[b] = r;
}

__global__ __launch_bounds__(RES_THREADS) void k_res_stage(ResStageArgs a)
{
    const int b = blockIdx.y, i = blockIdx.x * RES_THREADS + threadIdx.x, nm = a.f.n_max;
    const ResItem src = res_item(a.f, b, 0);
    if (i >= res_clamp(*src.n, nm)) return;
    const size_t s = (size_t)b * nm + (size_t)i;
    a.kps[s] = src.px[i];
    a.lmid[s] = src.lmid[i];
    a.is3d[s] = src.is3d[i];
    a.wpt[3 * s] = src.wpt[3 * i]; a.wpt[3 * s + 1] = src.wpt[3 * i + 1]; a.wpt[3 * s + 2] = src.wpt[3 * i + 2];
    a.scale[s] = 0;
}

__global__ __launch_bounds__(RES_THREADS) void k_res_carry(ResCarryArgs a)
{
    __shared__ int s_w[2][RES_WAVES];
    const int b = blockIdx.x, t = threadIdx.x, nm = a.f.n_max;
    const size_t o = (size_t)b * nm;
    const ResItem dst = res_item(a.f, b, 1);
    const int n = res_keep_count(a.pose_out, a.n_dev, b, nm);
    int m = 0;
    for (int i0 = 0, round = 0; i0 < n; i0 += RES_THREADS, round++) {
        const int i = i0 + t;
        const size_t s = o + (size_t)i;
        const bool keep = i < n && res_keep(a.status, a.epi_removed, a.pose_removed, s);
        int lm = 0; float2 px = make_float2(0.f, 0.f); double w0 = 0., w1 = 0., w2 = 0.; uint8_t d3 = 0;
        if (keep) { lm = a.lmid[s]; px = a.out_xy[s]; d3 = (uint8_t)(a.is3d[s] != 0); w0 = a.wpt[3 * s]; w1 = a.wpt[3 * s + 1]; w2 = a.wpt[3 * s + 2]; }
        const int r = res_rank(keep, round, s_w, m);                            // r <= i < n_max
        if (keep) { dst.lmid[r] = lm; dst.px[r] = px; dst.is3d[r] = d3; dst.wpt[3 * r] = w0; dst.wpt[3 * r + 1] = w1; dst.wpt[3 * r + 2] = w2; }
    }
    if (t == 0) *dst.n = m;
}

__global__ __launch_bounds__(RES_THREADS) void k_res_ckf_in(ResCkfArgs a)
{
    const int b = blockIdx.x, nm = a.f.n_max;
    if (!a.flag[b]) return;
    const size_t o = (size_t)b * nm;
    const ResItem src = res_item(a.f, b, 0);
    const int n = res_clamp(*src.n, nm);
    for (int i = threadIdx.x; i < n; i += RES_THREADS) { a.px[o + i] = src.px[i]; a.lmid[o + i] = src.lmid[i]; a.is3d[o + i] = src.is3d[i]; }
}

__global__ __launch_bounds__(RES_THREADS) void k_res_adopt(ResCkfArgs a)
{
    const int b = blockIdx.x, nm = a.f.n_max;
    if (!a.flag[b] || a.rec[b].action != OV2_CKF_CREATED) return;
    const size_t o = (size_t)b * nm;
    const ResItem src = res_item(a.f, b, 0), dst = res_item(a.f, b, 1);
    const int n_kf = res_clamp(a.rec[b].n_kf, nm), n_prev = res_clamp(a.rec[b].n_prev, n_kf);
    for (int i = threadIdx.x; i < n_kf; i += RES_THREADS) {
        const bool old = i < n_prev;
        dst.px[i] = a.px[o + i];
        dst.lmid[i] = a.lmid[o + i];
        dst.is3d[i] = old ? (uint8_t)(src.is3d[i] != 0) : (uint8_t)0;
        dst.wpt[3 * i] = old ? src.wpt[3 * i] : 0.; dst.wpt[3 * i + 1] = old ? src.wpt[3 * i + 1] : 0.; dst.wpt[3 * i + 2] = old ? src.wpt[3 * i + 2] : 0.;
    }
    if (threadIdx.x == 0) *dst.n = n_kf;
}

int ov2_launch_res_update(hipStream_t s, const ResUpdateArgs &a, int item0, int n_items, int ops_cap)
{
    hipLaunchKernelGGL(k_res_update, dim3(n_items), dim3(RES_THREADS), 0, s, a, item0, ops_cap);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

int ov2_launch_res_stage(hipStream_t s, const ResStageArgs &a, int n_active)
{
    hipLaunchKernelGGL(k_res_stage, dim3((a.f.n_max + RES_THREADS - 1) / RES_THREADS, n_active), dim3(RES_THREADS), 0, s, a);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

int ov2_launch_res_carry(hipStream_t s, const ResCarryArgs &a, int n_active)
{
    hipLaunchKernelGGL(k_res_carry, dim3(n_active), dim3(RES_THREADS), 0, s, a);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

int ov2_launch_res_ckf_in(hipStream_t s, const ResCkfArgs &a, int n_active)
{
    hipLaunchKernelGGL(k_res_ckf_in, dim3(n_active), dim3(RES_THREADS), 0, s, a);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

int ov2_launch_res_adopt(hipStream_t s, const ResCkfArgs &a, int n_active)
{
    hipLaunchKernelGGL(k_res_adopt, dim3(n_active), dim3(RES_THREADS), 0, s, a);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}
