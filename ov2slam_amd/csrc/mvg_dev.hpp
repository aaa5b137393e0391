// mvg_dev.hpp -- small fp64 geometry shared by triangulate.hip, mapmatch.hip, stereo.hip and fkf.hip: Sophus' SO3 / SE3 products
// and actions on a pose as held (restated from the vendored so3.hpp, se3.hpp), Eigen's quaternion-to-matrix, a serial 3x3
// matrix-vector product, CameraCalibration::projectCamToImage, cv::norm of a Point2f difference,
// MultiViewGeometry::computeSampsonDistance and the pose of a model (Eigen's matrix-to-quaternion branches; pnp.hip and epifilter.hip).
// Sums of three products run serially.
#pragma once
#include "common.hpp"

#pragma clang fp contract(off)

struct TriD3 { double x, y, z; };
struct TriQ { double x, y, z, w; };
struct TriSE3 { TriD3 t; TriQ q; };      // a pose as held: [tx ty tz qx qy qz qw]

// triangulate.hip: k_triangulate on device arrays (items_d: {first slot, count, first source row, 0} per item)
int ov2_launch_triangulate(hipStream_t s, const ov2_tri_params *params, const void *items_d, const double *twc_d, const double *srcT_d,
                           const float *unpx_d, const double *bv_d, const float *runpx_d, const double *rbv_d, const float *src_unpx_d,
                           const double *src_bv_d, const int *src_d, const uint8_t *is_stereo_d, uint8_t *status_d, double *wpt_d,
                           double *invdepth_d, int n_max, int n_items);

__device__ __forceinline__ double tri_dot(TriD3 a, TriD3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ TriD3 tri_cross(TriD3 a, TriD3 b)       // Eigen's cross
{
    return TriD3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
// SO3's constructor normalises (so3.hpp:297-303, :483-489); squaredNorm in serial order
__device__ __forceinline__ TriQ tri_qnormalize(double x, double y, double z, double w)
{
    const double n = sqrt(((x * x + y * y) + z * z) + w * w);
    return TriQ{x / n, y / n, z / n, w / n};
}
__device__ __forceinline__ TriQ tri_qmul(TriQ a, TriQ b)           // so3.hpp:329-343
{
    return tri_qnormalize(a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
                          a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z,
                          a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x,
                          a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z);
}
__device__ __forceinline__ TriD3 tri_qact(TriQ q, TriD3 p)         // so3.hpp:362-371
{
    const TriD3 qv{q.x, q.y, q.z};
    TriD3 uv = tri_cross(qv, p);
    uv = TriD3{uv.x + uv.x, uv.y + uv.y, uv.z + uv.z};
    const TriD3 c = tri_cross(qv, uv);
    return TriD3{(p.x + q.w * uv.x) + c.x, (p.y + q.w * uv.y) + c.y, (p.z + q.w * uv.z) + c.z};
}
__device__ __forceinline__ TriD3 tri_act(const TriSE3 &T, TriD3 p)   // se3.hpp:325-328
{
    const TriD3 r = tri_qact(T.q, p);
    return TriD3{r.x + T.t.x, r.y + T.t.y, r.z + T.t.z};
}
__device__ __forceinline__ TriSE3 tri_mul(const TriSE3 &A, const TriSE3 &B)   // se3.hpp:308-312
{
    const TriD3 r = tri_qact(A.q, B.t);
    return TriSE3{TriD3{A.t.x + r.x, A.t.y + r.y, A.t.z + r.z}, tri_qmul(A.q, B.q)};
}
__device__ __host__ __forceinline__ TriSE3 tri_load(const double *T)   // [tx ty tz qx qy qz qw] as held, no renormalisation
{
    return TriSE3{TriD3{T[0], T[1], T[2]}, TriQ{T[3], T[4], T[5], T[6]}};
}

// Eigen's toRotationMatrix, no renormalisation (row-major)
__device__ __forceinline__ void tri_rotmat(TriQ q, double R[9])
{
    const double tx = 2. * q.x, ty = 2. * q.y, tz = 2. * q.z;
    const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
    const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
    const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
    R[0] = 1. - (tyy + tzz); R[1] = txy - twz;        R[2] = txz + twy;
    R[3] = txy + twz;        R[4] = 1. - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy;        R[7] = tyz + twx;        R[8] = 1. - (txx + tyy);
}
__device__ __forceinline__ TriD3 tri_matvec(const double R[9], TriD3 v)
{
    return TriD3{(R[0] * v.x + R[1] * v.y) + R[2] * v.z, (R[3] * v.x + R[4] * v.y) + R[5] * v.z, (R[6] * v.x + R[7] * v.y) + R[8] * v.z};
}
// CameraCalibration::projectCamToImage (src/camera_calibration.cpp:243-252): double math, cv::Point2f result
__device__ __forceinline__ float2 tri_project(const double K[4], TriD3 p)
{
    const double invz = 1. / p.z;
    const double x = p.x * invz, y = p.y * invz;
    return make_float2((float)(K[0] * x + K[2]), (float)(K[1] * y + K[3]));
}
// cv::norm(a - b) of two cv::Point2f: the difference in float, the norm in double
__device__ __forceinline__ double tri_pdist(float2 a, float2 b)
{
    const float dx = a.x - b.x, dy = a.y - b.y;
    return sqrt((double)dx * (double)dx + (double)dy * (double)dy);
}

// float Sampson distance exactly as MultiViewGeometry::computeSampsonDistance narrows its doubles
__device__ __forceinline__ float sampson(const double *F, float lx, float ly, float rx, float ry)
{
    const double l[3] = {(double)lx, (double)ly, 1.}, r[3] = {(double)rx, (double)ry, 1.};
    double rtF[3], Fl[3], Ftr[3];
#pragma unroll
    for (int j = 0; j < 3; j++) rtF[j] = (r[0] * F[j] + r[1] * F[3 + j]) + r[2] * F[6 + j];
    float num = (float)((rtF[0] * l[0] + rtF[1] * l[1]) + rtF[2] * l[2]);
    num *= num;
#pragma unroll
    for (int k = 0; k < 3; k++) Fl[k] = (F[3 * k] * l[0] + F[3 * k + 1] * l[1]) + F[3 * k + 2] * l[2];
#pragma unroll
    for (int j = 0; j < 3; j++) Ftr[j] = (F[j] * r[0] + F[3 + j] * r[1]) + F[6 + j] * r[2];
    const float x1 = (float)Ftr[0], x2 = (float)Fl[0], y1 = (float)Ftr[1], y2 = (float)Fl[1];
    const float den = x1 * x1 + y1 * y1 + x2 * x2 + y2 * y2;
    return sqrtf(num / den);
}

// [t q] of (Rwc row-major | twc): Eigen's QuaternionBase::operator=(Matrix3) branches, then a normalisation
__host__ __device__ static inline void pose_from_model(const double *m, double *p)
{
    const double t = (m[0] + m[4]) + m[8];
    double q[4];                                                    // x y z w
    if (t > 0.0) {
        double s = sqrt(t + 1.0);
        q[3] = 0.5 * s; s = 0.5 / s;
        q[0] = (m[7] - m[5]) * s; q[1] = (m[2] - m[6]) * s; q[2] = (m[3] - m[1]) * s;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[4 * i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        double s = sqrt(((m[4 * i] - m[4 * j]) - m[4 * k]) + 1.0);
        q[i] = 0.5 * s; s = 0.5 / s;
        q[3] = (m[3 * k + j] - m[3 * j + k]) * s;
        q[j] = (m[3 * j + i] + m[3 * i + j]) * s;
        q[k] = (m[3 * k + i] + m[3 * i + k]) * s;
    }
    const double nq = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    p[0] = m[9]; p[1] = m[10]; p[2] = m[11];
    p[3] = q[0] / nq; p[4] = q[1] / nq; p[5] = q[2] / nq; p[6] = q[3] / nq;
}
