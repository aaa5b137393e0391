// lkw.hip -- VisualFrontEnd::kltTracking for ONE camera frame: a whole wavefront per keypoint (gfx950, wave64).
//
// Same arithmetic and the same reference semantics as lk.hip / lk3.hip (cv::calcOpticalFlowPyrLK inside
// FeatureTracker::fbKltTracking, /root/reference/src/feature_tracker.cpp:35-137; both calls and the retry of
// VisualFrontEnd::kltTracking, src/visual_front_end.cpp:132-275; the stereo variant of MapManager::stereoMatching,
// src/map_manager.cpp:497-565), different work mapping.  A single frame has ~300 keypoints on 1024 SIMDs: nothing is
// throughput-bound, the frame's latency is every keypoint's own dependent chain -- ~5 level visits of (global round trip ->
// template build -> ~4 Gauss-Newton trips).  k_track_klt (lk.hip) gives a keypoint 16 lanes (lane = window row, 9 pixels per
// lane): ~240 dependent wave-instructions per trip.  Here the 81 window pixels are spread over all 64 lanes (pixels p and
// p + 64), so a trip is ~2 pixels of work per lane + two wave reductions:
//   * both neighbourhoods of a level are staged in LDS by the whole wavefront (one dword per lane and row segment), the
//     Scharr derivative is evaluated once on the 10 x 10 integer grid the bilinear footprints touch (one position per lane),
//   * integer partial sums are reduced exactly: 4 DPP steps inside each 16-lane row (|row sum| < 2^31), the four row totals
//     through v_readlane in fp64 -- bit-identical to the oracle's int64 accumulation,
//   * one keypoint per wavefront: every branch (level skip, re-centring fetch, convergence) is wave-uniform.
// The search block of the NEXT level is requested while the current level iterates (its position is predicted from the current
// estimate; the +-3-pixel margin of the block absorbs the rest, and the ordinary re-centring fetch is the fall-back).
#include "lkw_dev.hpp"

// VisualFrontEnd::kltTracking / the LK part of MapManager::stereoMatching in ONE launch: same contract as k_track_klt (lk.hip)
template <bool FACC>
__global__ __launch_bounds__(64) void k_track_klt_w(PyrDesc P, PyrDesc C, LKParams prm, int lvl_prior, int lvl_full,
                                                    const int *__restrict__ n_dev, const float2 *__restrict__ kps,
                                                    const float2 *__restrict__ priors, const uint8_t *__restrict__ flags,
                                                    float2 *__restrict__ out_xy, uint8_t *__restrict__ status,
                                                    int *__restrict__ iters_out, const float *__restrict__ sad_x, float sad_up)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds[W_LDS_INT + (FACC ? 2 * W_FACC_PIX : 0)];
    // blockIdx.y: batch item (lock-step tracker, trackb.hip: n_max point slots and one count per item; 0 for one camera)
    const int item = blockIdx.y;
    const int n = n_dev ? n_dev[item] : prm.n_max;
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= n) return;
    const int i = item * prm.n_max + blockIdx.x;
    const uint8_t *pb = P.base + (long long)item * P.item_stride, *cb = C.base + (long long)item * C.item_stride;
    const float2 kp = kps[i];
    float2 pr = priors[i];
    const bool has_prior = (flags[i] & 1) != 0;
    const bool stereo = sad_x != nullptr;
    if (stereo && !has_prior) {                                    // map_manager.cpp:433-437
        pr = kp;
        const float xp = sad_x[i] * sad_up;
        if (xp >= 0.f && xp <= kp.x) pr.x = xp;
    }
    int max_level = has_prior ? lvl_prior : lvl_full;
    int ok = 0, retried = 0, iters = 0;
    float fx = 0.f, fy = 0.f;
    for (int attempt = 0; attempt < 2; attempt++) {
        int it = 0;
        ok = w_fb_track_point<FACC>(pb, cb, P, C, prm, max_level, kp, pr, lane, lds, fx, fy, it);
        iters += it;
        if (ok || !has_prior || attempt == 1) break;
        pr = make_float2(fx, fy);                                   // visual_front_end.cpp:213-217, map_manager.cpp:533-538
        max_level = lvl_full; retried = 1;
    }
    if (lane == 0) {
        out_xy[i] = make_float2(fx, fy);
        status[i] = (uint8_t)(ok | (retried << 1));
        if (iters_out) iters_out[i] = iters;
    }
}

int ov2_launch_track_klt_w(hipStream_t s, const PyrDesc &P, const PyrDesc &C, const LKParams &prm, int lp, int lf, int n_max, const int *n_dev,
                           const float *kps, const float *priors, const uint8_t *flags, float *out_xy, uint8_t *status, int *iters,
                           const float *sad_x, float sad_up, int items, int lk_acc)
{
    if (lk_acc == OV2_LK_ACC_FLOAT_UI4)
        hipLaunchKernelGGL(k_track_klt_w<true>, dim3(n_max, items), dim3(64), 0, s, P, C, prm, lp, lf, n_dev, (const float2 *)kps, (const float2 *)priors, flags,
                           (float2 *)out_xy, status, iters, sad_x, sad_up);
    else
        hipLaunchKernelGGL(k_track_klt_w<false>, dim3(n_max, items), dim3(64), 0, s, P, C, prm, lp, lf, n_dev, (const float2 *)kps, (const float2 *)priors, flags,
                           (float2 *)out_xy, status, iters, sad_x, sad_up);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}
