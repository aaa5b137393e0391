// keypoint_dev.hpp -- device functions shared by keypoint.hip and stereo.hip: the reference's
// CameraCalibration::undistortImagePoint (src/camera_calibration.cpp:313-333) restated in fp64
// (cv::undistortPoints / cv::fisheye::undistortPoints with P = K), no FMA contraction.
#pragma once
#include "common.hpp"
#include <math.h>

#pragma clang fp contract(off)

struct KpCalib {
    double fx, fy, cx, cy;
    double k[14];
    double iK[9];
    int nD, model;
};

__device__ __forceinline__ void kp_undistort_pinhole(const KpCalib &c, double u, double v, double &ox, double &oy)
{
    const double ifx = 1. / c.fx, ify = 1. / c.fy;
    double x = (u - c.cx) * ifx, y = (v - c.cy) * ify;
    const double x0 = x, y0 = y;
    const double *k = c.k;
    for (int j = 0; j < 5; j++) {
        const double r2 = x * x + y * y;
        const double icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
        if (icdist < 0) { x = (u - c.cx) * ifx; y = (v - c.cy) * ify; break; }
        const double deltaX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2;
        const double deltaY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2;
        x = (x0 - deltaX) * icdist;
        y = (y0 - deltaY) * icdist;
    }
    const double xx = c.fx * x + 0. * y + c.cx, yy = 0. * x + c.fy * y + c.cy, ww = 1. / (0. * x + 0. * y + 1.);
    ox = xx * ww; oy = yy * ww;
}

__device__ __forceinline__ bool kp_undistort_fisheye(const KpCalib &c, double u, double v, double &ox, double &oy)
{
    const double EPS = 1e-8, PI_2 = 3.1415926535897932384626433832795 / 2.;
    const double pwx = (u - c.cx) / c.fx, pwy = (v - c.cy) / c.fy;
    double theta_d = sqrt(pwx * pwx + pwy * pwy);
    theta_d = fmin(fmax(-PI_2, theta_d), PI_2);
    bool converged = false;
    double theta = theta_d, scale = 0.0;
    if (fabs(theta_d) > EPS) {
        for (int j = 0; j < 10; j++) {
            const double theta2 = theta * theta, theta4 = theta2 * theta2, theta6 = theta4 * theta2, theta8 = theta6 * theta2;
            const double k0_theta2 = c.k[0] * theta2, k1_theta4 = c.k[1] * theta4, k2_theta6 = c.k[2] * theta6, k3_theta8 = c.k[3] * theta8;
            const double theta_fix = (theta * (1 + k0_theta2 + k1_theta4 + k2_theta6 + k3_theta8) - theta_d) /
                                     (1 + 3 * k0_theta2 + 5 * k1_theta4 + 7 * k2_theta6 + 9 * k3_theta8);
            theta = theta - theta_fix;
            if (fabs(theta_fix) < EPS) { converged = true; break; }
        }
        scale = tan(theta) / theta_d;
    } else converged = true;
    const bool flipped = (theta_d < 0 && theta > 0) || (theta_d > 0 && theta < 0);
    if (!converged || flipped) return false;
    const double pux = pwx * scale, puy = pwy * scale;
    const double prx = (0. + c.fx * pux) + 0. * puy + c.cx * 1.0;
    const double pry = (0. + 0. * pux) + c.fy * puy + c.cy * 1.0;
    const double prz = (0. + 0. * pux) + 0. * puy + 1. * 1.0;
    ox = prx / prz; oy = pry / prz;
    return true;
}


// host: validate and pack the calibration (defined in keypoint.hip)
int ov2_kp_calib(int model, const double K[4], const double *D, int nD, const double iK[9], KpCalib &c);
// keypoint.hip: k_compute_keypoints on device arrays, `items` items of n_max point slots and one n_dev entry each
int ov2_launch_compute_keypoints(hipStream_t s, const KpCalib &c, const float *px_d, int n_max, const int *n_dev, float *unpx_d, double *bv_d, int items = 1);
// priors.hip: k_prior_frame on device arrays with n_max point slots per item
int ov2_launch_prior_frame(hipStream_t s, const KpCalib &c, double img_w, double img_h, int use_prior, const void *items_d,
                           const double *Tcw_d, const float *px_d, const uint8_t *is3d_d, const double *wpt_d, float *prior_d,
                           uint8_t *has_prior_d, int n_max, int n_items);
// priors.hip: k_prior_stereo, and stereo.hip: k_line_min_sad / k_epipolar_check, on device arrays with n_max point slots per item
int ov2_launch_prior_stereo(hipStream_t s, const KpCalib &c, const double *Tcic0, double img_w, double img_h, int ncellsize, int nbw, int nbh,
                            int rect, const void *items_d, const double *Tcw_d, const float *px_d, const float *unpx_d, const double *bv_d,
                            const double *wpt_d, const uint8_t *state_d, const int *cell_start_d, const int *cell_kp_d, float *prior_d,
                            uint8_t *has_prior_d, uint8_t *skip_d, int n_max, int n_items);
int ov2_launch_line_min_sad(hipStream_t s, const ov2_pyr *left, const ov2_pyr *right, int level, int nwinsize, int go_left, const float *pts_d,
                            int n_max, float *xprior_d, float *l1err_d, const int *n_dev, int n_items);
int ov2_launch_epipolar_check(hipStream_t s, int rect, const double Frl[9], const KpCalib &c, const float *lunpx_d, float *rkps_d, int n_max,
                              float *runpx_d, float *epi_err_d, uint8_t *ok_d, const int *n_dev, int n_items);

// The forward model: CameraCalibration::projectCamToImageDist (src/camera_calibration.cpp:254-281) of a camera-frame point.
// x = X / z, y = Y / z in double through invz; without coefficients Point2f(fx x + cx, fy y + cy).  With coefficients x, y are
// first rounded to float (cv::Point3f / cv::Point2f), then cv::projectPoints with zero rotation and translation (pinhole: the
// radial-tangential-rational-thin-prism model, k = k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4, absent ones 0) or
// cv::fisheye::distortPoints, both in double, and the pixel is rounded to float.
__device__ __forceinline__ float2 kp_project_dist(const KpCalib &c, double X, double Y, double Z)
{
    const double invz = 1. / Z;
    double x = X * invz, y = Y * invz;
    if (c.nD <= 0) return make_float2((float)(c.fx * x + c.cx), (float)(c.fy * y + c.cy));
    x = (double)(float)x; y = (double)(float)y;
    const double *k = c.k;
    if (c.model == OV2_CAM_FISHEYE) {
        const double r = sqrt(x * x + y * y);
        const double theta = atan(r);
        const double theta2 = theta * theta, theta4 = theta2 * theta2, theta6 = theta4 * theta2, theta8 = theta4 * theta4;
        const double theta_d = theta * (1 + k[0] * theta2 + k[1] * theta4 + k[2] * theta6 + k[3] * theta8);
        const double cdist = r > 1e-8 ? theta_d * (1.0 / r) : 1;
        return make_float2((float)((x * cdist) * c.fx + c.cx), (float)((y * cdist) * c.fy + c.cy));
    }
    const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
    const double a1 = 2 * x * y, a2 = r2 + 2 * x * x, a3 = r2 + 2 * y * y;
    const double cdist = 1 + k[0] * r2 + k[1] * r4 + k[4] * r6;
    const double icdist2 = 1. / (1 + k[5] * r2 + k[6] * r4 + k[7] * r6);
    const double xd = x * cdist * icdist2 + k[2] * a1 + k[3] * a2 + k[8] * r2 + k[9] * r4;
    const double yd = y * cdist * icdist2 + k[2] * a3 + k[3] * a1 + k[10] * r2 + k[11] * r4;
    return make_float2((float)(xd * c.fx + c.cx), (float)(yd * c.fy + c.cy));
}

// undistortImagePoint on a float pixel: `return pt` when there is no distortion vector
__device__ __forceinline__ float2 kp_undistort_image_point(const KpCalib &c, float2 p)
{
    if (c.nD <= 0) return p;
    double ox, oy;
    if (c.model == OV2_CAM_FISHEYE) {
        if (kp_undistort_fisheye(c, (double)p.x, (double)p.y, ox, oy)) return make_float2((float)ox, (float)oy);
        return make_float2(-1000000.0f, -1000000.0f);
    }
    kp_undistort_pinhole(c, (double)p.x, (double)p.y, ox, oy);
    return make_float2((float)ox, (float)oy);
}
