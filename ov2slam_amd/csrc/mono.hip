// mono.hip -- the two kernels ov2_btracker_track_mono (trackb.hip) puts around the lock-step step of f18 / f16 on gfx950, so that the
// per-frame sequence of VisualFrontEnd::trackMono (src/visual_front_end.cpp:65-128) runs in one enqueue with the frame pose and the
// motion model resident on the device:
//   k_mono_apply   one lane per item, in front of k_prior_frame: applyMotionModel (motion_dev.hpp, the code of ov2_motion_apply) on
//                  the resident pose and state; the predicted pose goes where the step's pose chain reads it, its inverse where the
//                  priors read it.
//   k_mono_pack    ONE WORK-GROUP OF FOUR WAVEFRONTS PER ITEM, behind k_pose_unpack, the scheme of k_epif_pack (frameepi.hip): the
//                  slots that are tracked and were removed neither by the filter nor by the pose, in slot order -- the frame
//                  checkNewKfReq sees (:986-1061) --, packed with lmid, px, unpx, bv, is3d; empty where computePose reset the frame
//                  (:1181-1203).  Thread 0 then writes the item's record for k_fkf_parallax, runs updateMotionModel (the code of
//                  ov2_motion_update) on the pose record's Twc and stores the new resident pose and state.
// k_fkf_parallax itself (fkf.hip, ov2_launch_kf_decision) follows on the packed frame.  No atomics, no scratch, 32 bytes of LDS; every
// count read from device memory is clamped against n_max before it indexes anything.
#include "mono_dev.hpp"

#pragma clang fp contract(off)
#include "motion_dev.hpp"

#define MN_THREADS 256
#define MN_WAVES (MN_THREADS / 64)

static_assert(sizeof(FkfItemD) == 176, "FkfItemD layout");

__device__ __forceinline__ int mn_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__global__ __launch_bounds__(64) void k_mono_apply(MonoArgs a, int n_active)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= n_active) return;
    const ov2_motion_state si = a.r_st[b];
    double T[7], To[7], Ti[7];
#pragma unroll
    for (int k = 0; k < 7; k++) T[k] = a.r_T[7 * (size_t)b + k];
    ov2_motion_state so;
    uint8_t rs;
    mo_apply(si, T, a.time[b], so, To, Ti, &rs);
    a.sa[b] = so;
#pragma unroll
    for (int k = 0; k < 7; k++) { a.q_T[7 * (size_t)b + k] = To[k]; a.pT[7 * (size_t)b + k] = To[k]; a.m_T[7 * (size_t)b + k] = Ti[k]; }
    a.rs[b] = rs;
}

__global__ __launch_bounds__(MN_THREADS) void k_mono_pack(MonoArgs a)
{
    __shared__ int s_w[2][MN_WAVES];                               // the wavefronts' counts of a round; two sets, so one barrier a round
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6, nm = a.n_max;
    const size_t o = (size_t)b * nm;                                // the item's first slot, and its first packed keypoint (cur0)
    int n = 0;
    if (a.pose_out) {
        const int action = a.pose_out[b].action;
        n = (action == OV2_POSE_P3P_RESET || action == OV2_POSE_PNP_RESET) ? 0 : mn_clamp(a.n_dev[b], nm);     // resetFrame()
    }
    int m = 0;
    for (int i0 = 0, round = 0; i0 < n; i0 += MN_THREADS, round++) {
        const int i = i0 + t;
        const size_t s = o + (size_t)i;
        const bool keep = i < n && (a.status[s] & 3) == 1 && !(a.epi_removed && a.epi_removed[s] != 0) && a.pose_removed[s] == 0;
        int lm = 0; float2 px = make_float2(0.f, 0.f), un = make_float2(0.f, 0.f); double b0 = 0., b1 = 0., b2 = 0.; uint8_t d3 = 0;
        if (keep) { lm = a.lmid[s]; px = a.out_xy[s]; un = a.unpx[s]; b0 = a.bv[3 * s]; b1 = a.bv[3 * s + 1]; b2 = a.bv[3 * s + 2]; d3 = a.is3d[s]; }
        const unsigned long long mk = __ballot(keep);
        int *sw = s_w[round & 1];
        if (lane == 0) sw[wave] = __popcll(mk);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < MN_WAVES; w++) { const int c = sw[w]; all += c; before += w < wave ? c : 0; }
        if (keep) {
            const int r = m + before + __popcll(mk & ((1ull << lane) - 1ull));     // r <= i < n_max
            const size_t d = o + (size_t)r;
            a.c_lmid[d] = lm; a.c_px[d] = px; a.c_unpx[d] = un; a.c_bv[3 * d] = b0; a.c_bv[3 * d + 1] = b1; a.c_bv[3 * d + 2] = b2;
            a.c_is3d[d] = (uint8_t)(d3 != 0);
        }
        m += all;
    }
    if (t != 0) return;
    double Tw[7];
#pragma unroll
    for (int k = 0; k < 7; k++) Tw[k] = a.pose_out ? a.pose_out[b].Twc[k] : a.q_T[7 * (size_t)b + k];
    const FeKfHdr &h = a.hdr[b];
    const MonoKfInfo ki = a.r_ki[b];
    FkfItemD it;
    it.cur0 = (int)o; it.n_cur = m; it.kf0 = (int)o; it.n_kf = mn_clamp(h.n_kf, nm);
    it.cur_id = a.frame_id[b]; it.kf_id = ki.kf_id; it.kf_nb3dkps = ki.kf_nb3dkps; it.localba_is_on = a.localba[b];
    it.noccupcells = -1; it.nb3dkps = -1; it.pad0 = 0; it.pad1 = 0;
    it.cur_time = a.time[b]; it.kf_time = a.r_kt[b];
#pragma unroll
    for (int k = 0; k < 7; k++) { it.cur_Twc[k] = Tw[k]; it.kf_Tcw[k] = h.kf_Tcw[k]; }
    a.items[b] = it;
    a.ncur_io[b] = m;
    const ov2_motion_state si = a.sa[b];
    ov2_motion_state so;
    mo_update(si, Tw, a.time[b], so);
    a.su[b] = so;
    a.r_st[b] = so;
#pragma unroll
    for (int k = 0; k < 7; k++) a.r_T[7 * (size_t)b + k] = Tw[k];
}

int ov2_launch_mono_apply(hipStream_t s, const MonoArgs &a, int n_active)
{
    hipLaunchKernelGGL(k_mono_apply, dim3((n_active + 63) / 64), dim3(64), 0, s, a, n_active);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

int ov2_launch_mono_pack(hipStream_t s, const MonoArgs &a, int n_active)
{
    hipLaunchKernelGGL(k_mono_pack, dim3(n_active), dim3(MN_THREADS), 0, s, a);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}
