// motion.hip -- the constant-velocity MotionModel of the reference's include/visual_front_end.hpp (:38-90) for gfx950:
//   k_motion_apply    applyMotionModel (:43-58): the resync of prevTwc_ when the caller's pose moved away from it (a loop closure, a
//                     bundle adjustment), the prediction Twc * exp(log_relT * dt), and the inverse of the prediction (the Tcw the
//                     tracking priors project with) in the arithmetic of ov2_se3_inverse.
//   k_motion_update   updateMotionModel (:60-78): log(prevTwc^-1 * Twc) / dt, the first call only stores.
// Fp64, ONE LANE PER ITEM: an item is a few hundred flops with two or three sin / cos / atan; the call is a launch and two copies.
// The SE(3) arithmetic is se3_dev.hpp's (shared with posegraph.hip); include/ov2slam_hip.h states the rules, tests/motion_ref.py is
// the same in numpy.
#include "common.hpp"
#include <cmath>

#pragma clang fp contract(off)
#include "motion_dev.hpp"              // mo_apply, mo_update: the lock-step step (mono.hip) runs them too

#define MO_THREADS 64
static_assert(sizeof(ov2_motion_state) == 112, "ov2_motion_state layout");

__global__ __launch_bounds__(MO_THREADS) void k_motion_apply(int n, const ov2_motion_state *__restrict__ state_in,
                                                             const double *__restrict__ Twc_in, const double *__restrict__ time,
                                                             ov2_motion_state *__restrict__ state_out, double *__restrict__ Twc_out,
                                                             double *__restrict__ Tcw_out, uint8_t *__restrict__ resynced)
{
    const int b = blockIdx.x * MO_THREADS + threadIdx.x;
    if (b >= n) return;
    const ov2_motion_state si = state_in[b];
    double T[7], To[7], Ti[7];
#pragma unroll
    for (int k = 0; k < 7; k++) T[k] = Twc_in[7 * (size_t)b + k];
    ov2_motion_state so;
    uint8_t rs;
    mo_apply(si, T, time[b], so, To, Ti, &rs);
    state_out[b] = so;
#pragma unroll
    for (int k = 0; k < 7; k++) { Twc_out[7 * (size_t)b + k] = To[k]; Tcw_out[7 * (size_t)b + k] = Ti[k]; }
    resynced[b] = rs;
}

__global__ __launch_bounds__(MO_THREADS) void k_motion_update(int n, const ov2_motion_state *__restrict__ state_in,
                                                              const double *__restrict__ Twc, const double *__restrict__ time,
                                                              ov2_motion_state *__restrict__ state_out)
{
    const int b = blockIdx.x * MO_THREADS + threadIdx.x;
    if (b >= n) return;
    const ov2_motion_state si = state_in[b];
    double T[7];
#pragma unroll
    for (int k = 0; k < 7; k++) T[k] = Twc[7 * (size_t)b + k];
    ov2_motion_state so;
    mo_update(si, T, time[b], so);
    state_out[b] = so;
}

static bool mo_finite(const double *v, int n)
{
    for (int k = 0; k < n; k++)
        if (!std::isfinite(v[k])) return false;
    return true;
}

// every input check of the four entry points, before the context is looked at
static int mo_check(int n, const ov2_motion_state *state_in, const double *Twc, const double *time)
{
    OV2_REQUIRE(n >= 0, OV2_EINVAL, "n < 0");
    OV2_REQUIRE(n == 0 || (state_in && Twc && time), OV2_EINVAL, "NULL array (state_in / Twc / time)");
    for (int b = 0; b < n; b++) {
        const ov2_motion_state &s = state_in[b];
        OV2_REQUIRE(std::isfinite(s.prev_time) && mo_finite(s.prevTwc, 7) && mo_finite(s.log_relT, 6), OV2_EINVAL,
                    "motion state that is not finite");
        OV2_REQUIRE(mo_finite(Twc + 7 * (size_t)b, 7) && std::isfinite(time[b]), OV2_EINVAL, "pose or time that is not finite");
        OV2_REQUIRE(!(s.prev_time >= 0. && time[b] <= s.prev_time), OV2_EINVAL,
                    "time is not after the state's prev_time (the reference exits on dt < 0 and divides by dt == 0)");
    }
    return OV2_OK;
}

// staging: [state_in 112][Twc 56][time 8] per item up, [state_out 112] (apply: [Twc_out 56][Tcw_out 56][resynced 1]) per item down
static int mo_run(ov2_ctx *ctx, bool apply, int n, const ov2_motion_state *state_in, const double *Twc, const double *time,
                  ov2_motion_state *state_out, double *Twc_out, double *Tcw_out, uint8_t *resynced)
{
    int rc = mo_check(n, state_in, Twc, time);
    if (rc) return rc;
    OV2_REQUIRE(n == 0 || state_out, OV2_EINVAL, "NULL state_out");
    if (apply) OV2_REQUIRE(n == 0 || (Twc_out && Tcw_out && resynced), OV2_EINVAL, "NULL array (Twc_out / Tcw_out / resynced)");
    OV2_REQUIRE(ctx, OV2_EINVAL, "NULL context");
    if (n == 0) return OV2_OK;
    const size_t B = (size_t)n;
    StageCursor c(16);
    const size_t o_si = c.take(sizeof(ov2_motion_state) * B), o_T = c.take(56 * B), o_tm = c.take(8 * B);
    const size_t o_so = c.take(sizeof(ov2_motion_state) * B), o_To = c.take(apply ? 56 * B : 0), o_Ti = c.take(apply ? 56 * B : 0);
    const size_t o_rs = c.take(apply ? B : 0), total = c.off;
    Stage st;
    rc = st.open(ctx, total, total);  if (rc) return rc;
    uint8_t *hs = st.h, *ds = st.d;
    memcpy(hs + o_si, state_in, sizeof(ov2_motion_state) * B);
    memcpy(hs + o_T, Twc, 56 * B);
    memcpy(hs + o_tm, time, 8 * B);
    rc = st.upload(0, o_so);  if (rc) return rc;
    const dim3 grid((n + MO_THREADS - 1) / MO_THREADS), block(MO_THREADS);
    if (apply)
        hipLaunchKernelGGL(k_motion_apply, grid, block, 0, ctx->stream, n, (const ov2_motion_state *)(ds + o_si), (const double *)(ds + o_T),
                           (const double *)(ds + o_tm), (ov2_motion_state *)(ds + o_so), (double *)(ds + o_To), (double *)(ds + o_Ti),
                           ds + o_rs);
    else
        hipLaunchKernelGGL(k_motion_update, grid, block, 0, ctx->stream, n, (const ov2_motion_state *)(ds + o_si), (const double *)(ds + o_T),
                           (const double *)(ds + o_tm), (ov2_motion_state *)(ds + o_so));
    OV2_HIP_CHECK(hipGetLastError());
    rc = st.download(o_so, total, o_so);  if (rc) return rc;
    rc = st.sync();  if (rc) return rc;
    memcpy(state_out, hs + o_so, sizeof(ov2_motion_state) * B);
    if (apply) {
        memcpy(Twc_out, hs + o_To, 56 * B);
        memcpy(Tcw_out, hs + o_Ti, 56 * B);
        memcpy(resynced, hs + o_rs, B);
    }
    return OV2_OK;
}

extern "C" {

int ov2_motion_apply_batch(ov2_ctx *ctx, int n, const ov2_motion_state *state_in, const double *Twc_in, const double *time,
                           ov2_motion_state *state_out, double *Twc_out, double *Tcw_out, uint8_t *resynced)
{
    return mo_run(ctx, true, n, state_in, Twc_in, time, state_out, Twc_out, Tcw_out, resynced);
}

int ov2_motion_apply(ov2_ctx *ctx, const ov2_motion_state *state_in, const double Twc_in[7], double time, ov2_motion_state *state_out,
                     double Twc_out[7], double Tcw_out[7], uint8_t *resynced)
{
    return mo_run(ctx, true, 1, state_in, Twc_in, &time, state_out, Twc_out, Tcw_out, resynced);
}

int ov2_motion_update_batch(ov2_ctx *ctx, int n, const ov2_motion_state *state_in, const double *Twc, const double *time,
                            ov2_motion_state *state_out)
{
    return mo_run(ctx, false, n, state_in, Twc, time, state_out, nullptr, nullptr, nullptr);
}

int ov2_motion_update(ov2_ctx *ctx, const ov2_motion_state *state_in, const double Twc[7], double time, ov2_motion_state *state_out)
{
    return mo_run(ctx, false, 1, state_in, Twc, &time, state_out, nullptr, nullptr, nullptr);
}

}
