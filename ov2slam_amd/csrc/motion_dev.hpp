// motion_dev.hpp -- the motion model on one item, as device functions: motion.hip (ov2_motion_apply / ov2_motion_update) and mono.hip
// (the lock-step step ov2_btracker_track_mono) run the same code, so the step's bits are the standalone calls'.
// Include AFTER the file's `#pragma clang fp contract(off)` (se3_dev.hpp's rule).
#pragma once
#include "se3_dev.hpp"
#include "frameepi_dev.hpp"            // fe_invert_hd: the host arithmetic of ov2_se3_inverse, on the device

#define MO_RESYNC_PREC 1e-5            // Eigen's isZero(1.e-5), :48

// applyMotionModel on one item.  so aliases nothing the function still reads: the caller passes its own copy of the state.
__device__ __forceinline__ void mo_apply(const ov2_motion_state &si, const double *Twc, double time, ov2_motion_state &so,
                                         double *Twc_out, double *Tcw_out, uint8_t *resynced)
{
    so = si;
    uint8_t rs = 0;
    if (si.prev_time > 0.) {
        const PgSE3 T = pg_load(Twc);
        double d[6];
        pg_log(pg_mul(T, pg_inv(pg_load(si.prevTwc))), d);
        bool zero = true;                                   // isZero: every |d_k| <= prec; a NaN is not
#pragma unroll
        for (int k = 0; k < 6; k++) zero = zero && fabs(d[k]) <= MO_RESYNC_PREC;
        if (!zero) {
            rs = 1;
#pragma unroll
            for (int k = 0; k < 7; k++) so.prevTwc[k] = Twc[k];
        }
        const double dt = time - si.prev_time;
        double v[6];
#pragma unroll
        for (int k = 0; k < 6; k++) v[k] = si.log_relT[k] * dt;
        pg_store(pg_mul(T, pg_exp(v)), Twc_out);
    } else {
#pragma unroll
        for (int k = 0; k < 7; k++) Twc_out[k] = Twc[k];
    }
    fe_invert_hd(Twc_out, Tcw_out);
    *resynced = rs;
}

// updateMotionModel on one item
__device__ __forceinline__ void mo_update(const ov2_motion_state &si, const double *Twc, double time, ov2_motion_state &so)
{
    so = si;
    if (!(si.prev_time < 0.)) {
        const double dt = time - si.prev_time;
        double v[6];
        pg_log(pg_mul(pg_inv(pg_load(si.prevTwc)), pg_load(Twc)), v);
#pragma unroll
        for (int k = 0; k < 6; k++) so.log_relT[k] = v[k] / dt;
    }
    so.prev_time = time;
#pragma unroll
    for (int k = 0; k < 7; k++) so.prevTwc[k] = Twc[k];
}
