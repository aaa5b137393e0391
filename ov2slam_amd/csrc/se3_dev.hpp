// se3_dev.hpp -- SE(3) as Sophus::SE3d computes it, on the device, in fp64: the product, the inverse, log and exp.  posegraph.hip
// (the factor and Exp(delta) T of the pose-graph solver) and motion.hip (the constant-velocity motion model) share these functions:
// there is ONE copy, pinned to the reference's compiled code through tests/posegraph_ref.py (tests/test_posegraph_reference.py).
//
// Floating point: nothing here sets a contraction mode.  A file includes this header AFTER its own file-scope
// `#pragma clang fp contract(off)`, which then governs these functions too (the rule of ba_core.hpp, which it needs for d_quat_to_R).
#pragma once
#include "ba_core.hpp"
#include <cmath>

#define PG_EPS 1e-10              // Sophus::Constants<double>::epsilon()

struct PgSE3 { double q[4], t[3]; };      // q = (x, y, z, w), unit

__device__ __forceinline__ void pg_qnormalize(double *q)
{
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n;
}

__device__ __forceinline__ PgSE3 pg_load(const double *p)
{
    PgSE3 T;
    T.t[0] = p[0]; T.t[1] = p[1]; T.t[2] = p[2];
    T.q[0] = p[3]; T.q[1] = p[4]; T.q[2] = p[5]; T.q[3] = p[6];
    pg_qnormalize(T.q);                                    // Sophus::SE3d(q, t) normalises
    return T;
}

__device__ __forceinline__ void pg_rot(const double *q, const double *v, double *o)
{
    double R[9];
    d_quat_to_R(q, R);
#pragma unroll
    for (int i = 0; i < 3; i++) o[i] = R[3 * i] * v[0] + R[3 * i + 1] * v[1] + R[3 * i + 2] * v[2];
}

// a * b: the quaternion product of so3.hpp:329-343, renormalised (SO3's constructor)
__device__ __forceinline__ PgSE3 pg_mul(const PgSE3 &a, const PgSE3 &b)
{
    PgSE3 c;
    const double ax = a.q[0], ay = a.q[1], az = a.q[2], aw = a.q[3], bx = b.q[0], by = b.q[1], bz = b.q[2], bw = b.q[3];
    c.q[3] = aw * bw - ax * bx - ay * by - az * bz;
    c.q[0] = aw * bx + ax * bw + ay * bz - az * by;
    c.q[1] = aw * by + ay * bw + az * bx - ax * bz;
    c.q[2] = aw * bz + az * bw + ax * by - ay * bx;
    pg_qnormalize(c.q);
    double rt[3];
    pg_rot(a.q, b.t, rt);
    c.t[0] = a.t[0] + rt[0]; c.t[1] = a.t[1] + rt[1]; c.t[2] = a.t[2] + rt[2];
    return c;
}

__device__ __forceinline__ PgSE3 pg_inv(const PgSE3 &a)
{
    PgSE3 c;
    c.q[0] = -a.q[0]; c.q[1] = -a.q[1]; c.q[2] = -a.q[2]; c.q[3] = a.q[3];
    const double mt[3] = {-a.t[0], -a.t[1], -a.t[2]};
    pg_rot(c.q, mt, c.t);
    return c;
}

// Sophus SE3::log (se3.hpp:223-256, so3.hpp:247-290): v = [rho; omega]
__device__ __forceinline__ void pg_log(const PgSE3 &T, double *v)
{
    const double sn = T.q[0] * T.q[0] + T.q[1] * T.q[1] + T.q[2] * T.q[2], w = T.q[3];
    double k, theta;
    if (sn < PG_EPS * PG_EPS) {
        k = 2.0 / w - (2.0 / 3.0) * sn / (w * (w * w));
        theta = 2.0 * sn / w;
    } else {
        const double n = sqrt(sn);
        if (fabs(w) < PG_EPS) k = (w > 0.0 ? M_PI : -M_PI) / n;
        else k = 2.0 * atan(n / w) / n;
        theta = k * n;
    }
    const double om[3] = {k * T.q[0], k * T.q[1], k * T.q[2]};
    const double Om[9] = {0, -om[2], om[1], om[2], 0, -om[0], -om[1], om[0], 0};
    double c;
    if (fabs(theta) < PG_EPS) c = 1.0 / 12.0;
    else { const double h = 0.5 * theta; c = (1.0 - theta * cos(h) / (2.0 * sin(h))) / (theta * theta); }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        double s = 0;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double o2 = Om[3 * i] * Om[j] + Om[3 * i + 1] * Om[3 + j] + Om[3 * i + 2] * Om[6 + j];
            const double vinv = (i == j ? 1.0 : 0.0) - 0.5 * Om[3 * i + j] + c * o2;
            s += vinv * T.t[j];
        }
        v[i] = s;
    }
    v[3] = om[0]; v[4] = om[1]; v[5] = om[2];
}

// Sophus SE3::exp of a = [upsilon; omega] (se3.hpp:763-784, so3.hpp:585-621; the form of ba.hip's d_se3_left_plus, here without
// contraction)
__device__ __forceinline__ PgSE3 pg_exp(const double *a)
{
    const double *om = a + 3;
    const double theta_sq = om[0] * om[0] + om[1] * om[1] + om[2] * om[2];
    double theta, imag, real;
    if (theta_sq < PG_EPS * PG_EPS) {
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
    PgSE3 E;
    E.q[0] = imag * om[0]; E.q[1] = imag * om[1]; E.q[2] = imag * om[2]; E.q[3] = real;
    double V[9];
    if (theta < PG_EPS) d_quat_to_R(E.q, V);
    else {
        const double O[9] = {0, -om[2], om[1], om[2], 0, -om[0], -om[1], om[0], 0};
        const double c1 = (1.0 - cos(theta)) / theta_sq, c2 = (theta - sin(theta)) / (theta_sq * theta);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const double o2 = O[3 * i] * O[j] + O[3 * i + 1] * O[3 + j] + O[3 * i + 2] * O[6 + j];
                V[3 * i + j] = c1 * O[3 * i + j] + c2 * o2 + (i == j ? 1.0 : 0.0);
            }
    }
#pragma unroll
    for (int i = 0; i < 3; i++) E.t[i] = V[3 * i] * a[0] + V[3 * i + 1] * a[1] + V[3 * i + 2] * a[2];
    return E;
}

__device__ __forceinline__ void pg_store(const PgSE3 &T, double *out)
{
    out[0] = T.t[0]; out[1] = T.t[1]; out[2] = T.t[2];
    out[3] = T.q[0]; out[4] = T.q[1]; out[5] = T.q[2]; out[6] = T.q[3];
}
