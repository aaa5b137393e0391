// ba_pnp.hpp -- the device pieces of a pose-only (PnP) problem that more than one translation unit needs: the left-multiplicative
// SE(3) update and the reprojection residual of a fixed world point with its Jacobian.  Included by ba.hip (k_ba_pose_only and the
// multi-kernel solver) and pnp.hip (k_pnp_solve), after ba_core.hpp and after the file's own `#pragma clang fp contract(...)`,
// which governs these functions too.  The text is what ba.hip held before pnp.hip existed; d_residual_pnp only became generic in
// the type that carries the calibration (anything with a `double calib_l[4]`: fx fy cx cy).
#pragma once
#include "ba_core.hpp"

// T' = Exp(delta) * T   (se3left_parametrization.hpp:45-57, Sophus se3.hpp:763-784, so3.hpp:585-621)
__device__ void d_se3_left_plus(const double *pose, const double *a, double *out)
{
    const double *om = a + 3;
    const double theta_sq = om[0] * om[0] + om[1] * om[1] + om[2] * om[2];
    double theta, imag, real;
    if (theta_sq < 1e-10 * 1e-10) {
        theta = 0;
        const double t4 = theta_sq * theta_sq;
        imag = 0.5 - (1.0 / 48.0) * theta_sq + (1.0 / 3840.0) * t4;
        real = 1.0 - (1.0 / 8.0) * theta_sq + (1.0 / 384.0) * t4;
    } else {
        theta = sqrt(theta_sq);
        const double half = 0.5 * theta;
        imag = sin(half) / theta;
        real = cos(half);
    }
    const double qe[4] = {imag * om[0], imag * om[1], imag * om[2], real};
    double V[9], Re[9];
    d_quat_to_R(qe, Re);
    if (theta < 1e-10) {
        for (int k = 0; k < 9; k++) V[k] = Re[k];
    } else {
        const double O[9] = {0, -om[2], om[1], om[2], 0, -om[0], -om[1], om[0], 0};
        const double c1 = (1.0 - cos(theta)) / theta_sq, c2 = (theta - sin(theta)) / (theta_sq * theta);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                const double o2 = O[3 * i] * O[j] + O[3 * i + 1] * O[3 + j] + O[3 * i + 2] * O[6 + j];
                V[3 * i + j] = c1 * O[3 * i + j] + c2 * o2 + (i == j ? 1.0 : 0.0);
            }
    }
    double q[4] = {pose[3], pose[4], pose[5], pose[6]};
    const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    q[0] /= qn; q[1] /= qn; q[2] /= qn; q[3] /= qn;
    const double ax = qe[0], ay = qe[1], az = qe[2], aw = qe[3], bx = q[0], by = q[1], bz = q[2], bw = q[3];
    double r[4];
    r[3] = aw * bw - ax * bx - ay * by - az * bz;
    r[0] = aw * bx + ax * bw + ay * bz - az * by;
    r[1] = aw * by + ay * bw + az * bx - ax * bz;
    r[2] = aw * bz + az * bw + ax * by - ay * bx;
    const double rn = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3]);
    for (int i = 0; i < 3; i++)
        out[i] = V[3 * i] * a[0] + V[3 * i + 1] * a[1] + V[3 * i + 2] * a[2] +
                 Re[3 * i] * pose[0] + Re[3 * i + 1] * pose[1] + Re[3 * i + 2] * pose[2];
    out[3] = r[0] / rn; out[4] = r[1] / rn; out[5] = r[2] / rn; out[6] = r[3] / rn;
}

// DirectLeftSE3::ReprojectionErrorSE3 (ceres_parametrization.cpp:301-358): fixed world point, Jacobian w.r.t. the pose
template <bool JAC, class Dev>
__device__ __forceinline__ int d_residual_pnp(const Dev &D, const double *RTo, const double *xyz, const double *uv, double sigma,
                                              double *r, double *Jo)
{
    const double sqrt_info = 1.0 / sigma;
    const double d[3] = {xyz[0] - RTo[9], xyz[1] - RTo[10], xyz[2] - RTo[11]};
    double c[3];
    for (int i = 0; i < 3; i++) c[i] = RTo[i] * d[0] + RTo[3 + i] * d[1] + RTo[6 + i] * d[2];      // Rcw = Rwc^T
    const double invz = 1.0 / c[2];
    const double *K = D.calib_l;
    r[0] = sqrt_info * (K[0] * c[0] * invz + K[2] - uv[0]);
    r[1] = sqrt_info * (K[1] * c[1] * invz + K[3] - uv[1]);
    if (JAC) {
        const double invz2 = invz * invz;
        const double Jc[6] = {invz * K[0], 0, -c[0] * invz2 * K[0], 0, invz * K[1], -c[1] * invz2 * K[1]};
        double JR[6];
        for (int i = 0; i < 2; i++) for (int j = 0; j < 3; j++) JR[3 * i + j] = Jc[3 * i] * RTo[3 * j] + Jc[3 * i + 1] * RTo[3 * j + 1] + Jc[3 * i + 2] * RTo[3 * j + 2];
        const double S[9] = {0, -xyz[2], xyz[1], xyz[2], 0, -xyz[0], -xyz[1], xyz[0], 0};
        for (int i = 0; i < 2; i++)
            for (int j = 0; j < 3; j++) {
                const double jrs = JR[3 * i] * S[j] + JR[3 * i + 1] * S[3 + j] + JR[3 * i + 2] * S[6 + j];
                Jo[6 * i + j] = -sqrt_info * JR[3 * i + j];
                Jo[6 * i + 3 + j] = sqrt_info * jrs;
            }
    }
    return c[2] > 0;
}
