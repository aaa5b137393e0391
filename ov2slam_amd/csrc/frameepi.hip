// frameepi.hip -- epipolar2d2dFiltering inside the lock-step step on gfx950: what stands between k_pose_select and k_pose_pack
// (framepose.hip) when the tracker runs tracking, the filter and computePose in one enqueue (ov2_btracker_track_frame_epi_pose,
// trackb.hip).  The reference builds the filter's inputs on the host from the frame kltTracking left behind
// (src/visual_front_end.cpp:440-520) and removes the outliers from the frame before computePose reads it (:587-590).
//   k_epif_pack    ONE WORK-GROUP OF FOUR WAVEFRONTS PER ITEM, 256 slots a round: every lane reads its slot's status byte once and,
//                  where the keypoint was tracked, its lmid, unpx, bearing and 3-D flag -- consecutive lanes read consecutive
//                  records --; a ballot per wavefront and four counts in LDS give the stable, slot-ordered rank; the record goes to
//                  the epipolar block's current-frame arrays at item b's capacity slots (epif_dev.hpp), with the slot of every
//                  packed keypoint and the rank of every slot.  The first lanes then write the item's EpifItem from the resident
//                  keyframe header and the step's inputs (nb3dkps = -1: the chain counts the flags).
//   (epif_chain_enqueue: k_epif_gather, k_e5_solve, k_e5_score, k_e5_pick, k_epif_decide, untouched)
//   k_epif_apply   one lane per slot: removed / err from packed space to slot space through the ranks, pair_cur from packed
//                  indices to slots, the item's EpifOut to the step's result block, and THE SELECT BYTE OF EVERY REMOVED SLOT
//                  CLEARED, so that k_pose_pack sees the frame after the filter.
// No atomics, no scratch, 32 bytes of LDS.  Every count read from device memory is clamped against n_max before it indexes
// anything; a rank or a packed index is checked before it is used.
#include "frameepi_dev.hpp"

#pragma clang fp contract(off)

// threads of k_epif_pack's work-group.  Measured at 4096 items of 308 slots, two alternating passes: 64 (one wavefront
// per item, as k_pose_pack) 972 us, 256 947 us, 512 930 us -- the kernel waits for the host link, whose 48 MB it reads once
#define FE_THREADS 256
#define FE_WAVES (FE_THREADS / 64)

__device__ __forceinline__ int fe_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__global__ __launch_bounds__(FE_THREADS) void k_epif_pack(FeArgs a)
{
    __shared__ int s_w[2][FE_WAVES];                               // the wavefronts' counts of a round; two sets, so one barrier a round
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6, nm = a.n_max;
    const int n = fe_clamp(a.n_dev[b], nm);
    const size_t o = (size_t)b * nm;                                // the item's first slot, and its first packed keypoint (cur0)
    int m = 0;
    for (int i0 = 0, round = 0; i0 < n; i0 += FE_THREADS, round++) {
        const int i = i0 + t;
        const size_t s = o + (size_t)i;
        const bool keep = i < n && (a.status[s] & 3) == 1;
        int lm = 0; float2 un = make_float2(0.f, 0.f); double b0 = 0., b1 = 0., b2 = 0.; uint8_t d3 = 0;
        if (keep) { lm = a.lmid[s]; un = a.unpx[s]; b0 = a.bv[3 * s]; b1 = a.bv[3 * s + 1]; b2 = a.bv[3 * s + 2]; d3 = a.is3d[s]; }
        const unsigned long long mk = __ballot(keep);
        int *sw = s_w[round & 1];
        if (lane == 0) sw[wave] = __popcll(mk);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < FE_WAVES; w++) { const int c = sw[w]; all += c; before += w < wave ? c : 0; }
        if (keep) {
            const int r = m + before + __popcll(mk & ((1ull << lane) - 1ull));     // r <= i < n_max
            const size_t d = o + (size_t)r;
            a.c_lmid[d] = lm; a.c_unpx[d] = un; a.c_bv[3 * d] = b0; a.c_bv[3 * d + 1] = b1; a.c_bv[3 * d + 2] = b2;
            a.c_is3d[d] = (uint8_t)(d3 != 0);
            a.slot[d] = i;
            a.rank[s] = r;
        } else if (i < n) a.rank[s] = -1;
        m += all;
    }
    const FeKfHdr &h = a.hdr[b];
    EpifItem &it = a.items[b];
    if (t < 7) { it.cur_Twc[t] = a.Twc[7 * (size_t)b + t]; it.kf_Tcw[t] = h.kf_Tcw[t]; it.kf_Twc[t] = h.kf_Twc[t]; }
    if (t == 0) {
        it.cur0 = (int)o; it.n_cur = m; it.kf0 = (int)o; it.n_kf = fe_clamp(h.n_kf, nm);
        it.row0 = b * a.n_rows; it.n_rows = a.n_rows; it.nb3dkps = -1; it.nbkfs = a.nbkfs[b];
        it.seed = a.seed[b];
        a.ncur_io[b] = m;
    }
}

__global__ __launch_bounds__(256) void k_epif_apply(FeArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y, nm = a.n_max;
    const size_t o = (size_t)b * nm;
    if (blockIdx.x == 0 && threadIdx.x < (int)(sizeof(EpifOut) / 4))
        ((int *)(a.out_io + b))[threadIdx.x] = ((const int *)(a.out + b))[threadIdx.x];
    if (i >= fe_clamp(a.n_dev[b], nm)) return;
    const int r = a.rank[o + i];
    const bool in = r >= 0 && r < nm;
    const uint8_t rm = in ? a.removed[o + (size_t)r] : (uint8_t)0;
    a.removed_io[o + i] = rm;
    a.err_io[o + i] = in ? a.err[o + (size_t)r] : 0.f;
    if (rm != 0) a.sel[o + i] = 0;                                   // :587-590: gone from the frame before computePose reads it
    const int n_cur = fe_clamp(a.items[b].n_cur, nm), m = fe_clamp(a.out[b].m, n_cur);
    if (i < m) {                                                    // m <= n_cur <= n: lane i also moves match i
        const int pc = a.pair_cur[o + i];
        a.pair_io[o + i] = (unsigned)pc < (unsigned)n_cur ? a.slot[o + (size_t)pc] : -1;
    }
}

int ov2_frame_epi_hook(hipStream_t s, uint8_t *sel, void *arg)
{
    FeStep *st = (FeStep *)arg;
    FeArgs a = st->a;
    a.sel = sel;
    hipLaunchKernelGGL(k_epif_pack, dim3(st->n_active), dim3(FE_THREADS), 0, s, a);
    OV2_HIP_CHECK(hipGetLastError());
    const int rc = epif_chain_enqueue(s, st->params, st->L, st->block, st->n_active);
    if (rc != OV2_OK) return rc;
    hipLaunchKernelGGL(k_epif_apply, dim3((a.n_max + 255) / 256, st->n_active), dim3(256), 0, s, a);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

void ov2_fe_invert(const double T[7], double out[7])
{
    fe_invert_hd(T, out);
}

extern "C" int ov2_se3_inverse(const double T[7], double out[7])
{
    OV2_REQUIRE(T && out, OV2_EINVAL, "NULL argument");
    ov2_fe_invert(T, out);
    return OV2_OK;
}
