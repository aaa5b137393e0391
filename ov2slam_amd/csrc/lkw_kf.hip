// lkw_kf.hip -- VisualFrontEnd::kltTrackingFromKF for ONE camera frame, a whole wavefront per keypoint: the from-keyframe sibling of
// k_track_klt_w (lkw.hip) on the same device functions (lkw_dev.hpp).  A translation unit of its own: compiled next to k_track_klt_w
// it changed that kernel's register allocation (113 -> 115 and 103 -> 99 VGPRs), and the sibling is to stay as it is.
#include "lkw_dev.hpp"

// VisualFrontEnd::kltTrackingFromKF (src/visual_front_end.cpp:278-442) in ONE launch: k_track_klt_w's contract without the stereo
// inputs, plus retry_prior.  P is the keyframe's pyramid (kf_pyr_) and kps the keyframe's px_ of every slot (:336, :346).  A 3-D-prior
// slot that the one-level pass lost is retried on the full pyramid from retry_prior -- the frame's current px_ (:386), NOT the first
// pass's forward result as in kltTracking.  flag bit 1: the keyframe no longer holds the slot's lmid_ (:316-320): the slot is not
// tracked, status 4 (bit 2), its input px as output.
template <bool FACC>
__global__ __launch_bounds__(64) void k_track_klt_kf_w(PyrDesc P, PyrDesc C, LKParams prm, int lvl_prior, int lvl_full,
                                                       const int *__restrict__ n_dev, const float2 *__restrict__ kps,
                                                       const float2 *__restrict__ priors, const float2 *__restrict__ retry_prior,
                                                       const uint8_t *__restrict__ flags, float2 *__restrict__ out_xy,
                                                       uint8_t *__restrict__ status, int *__restrict__ iters_out)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds[W_LDS_INT + (FACC ? 2 * W_FACC_PIX : 0)];
    const int item = blockIdx.y;
    const int n = n_dev ? n_dev[item] : prm.n_max;
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= n) return;
    const int i = item * prm.n_max + blockIdx.x;
    const uint8_t *pb = P.base + (long long)item * P.item_stride, *cb = C.base + (long long)item * C.item_stride;
    const float2 kp = kps[i];
    const int fl = flags[i];
    if (fl & 2) {                                                   // wave-uniform: one slot per wavefront
        if (lane == 0) {
            out_xy[i] = kp;
            status[i] = 4;
            if (iters_out) iters_out[i] = 0;
        }
        return;
    }
    float2 pr = priors[i];
    const bool has_prior = (fl & 1) != 0;
    int max_level = has_prior ? lvl_prior : lvl_full;
    int ok = 0, retried = 0, iters = 0;
    float fx = 0.f, fy = 0.f;
    for (int attempt = 0; attempt < 2; attempt++) {
        int it = 0;
        ok = w_fb_track_point<FACC>(pb, cb, P, C, prm, max_level, kp, pr, lane, lds, fx, fy, it);
        iters += it;
        if (ok || !has_prior || attempt == 1) break;
        pr = retry_prior[i];                                        // visual_front_end.cpp:386
        max_level = lvl_full; retried = 1;
    }
    if (lane == 0) {
        out_xy[i] = make_float2(fx, fy);
        status[i] = (uint8_t)(ok | (retried << 1));
        if (iters_out) iters_out[i] = iters;
    }
}

int ov2_launch_track_klt_kf_w(hipStream_t s, const PyrDesc &P, const PyrDesc &C, const LKParams &prm, int lp, int lf, int n_max, const int *n_dev,
                              const float *kps, const float *priors, const float *retry_prior, const uint8_t *flags, float *out_xy,
                              uint8_t *status, int *iters, int items, int lk_acc)
{
    if (lk_acc == OV2_LK_ACC_FLOAT_UI4)
        hipLaunchKernelGGL(k_track_klt_kf_w<true>, dim3(n_max, items), dim3(64), 0, s, P, C, prm, lp, lf, n_dev, (const float2 *)kps, (const float2 *)priors,
                           (const float2 *)retry_prior, flags, (float2 *)out_xy, status, iters);
    else
        hipLaunchKernelGGL(k_track_klt_kf_w<false>, dim3(n_max, items), dim3(64), 0, s, P, C, prm, lp, lf, n_dev, (const float2 *)kps, (const float2 *)priors,
                           (const float2 *)retry_prior, flags, (float2 *)out_xy, status, iters);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}
