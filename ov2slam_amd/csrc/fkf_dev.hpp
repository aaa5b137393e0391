// fkf_dev.hpp -- the device functions of fkf.hip that epifilter.hip (epipolar2d2dFiltering) needs as well: the join
// (Frame::getKeypointById on ascending ids), the rotation of :489 / :1082-1084, the rotation-compensated distance of :514-517 and the
// serial widened float sum of :517.  One definition each: the chain's parallax IS ov2_parallax(unrot = 1, ., OV2_FKF_AVG_WIDE).
#pragma once
#include "mvg_dev.hpp"

#pragma clang fp contract(off)

// Frame::getKeypointById on ascending ids: the slot of `id`, -1 when the keyframe does not hold it
__device__ __forceinline__ int fkf_find(const int *kf, int n, int id)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (kf[mid] < id) lo = mid + 1; else hi = mid;
    }
    return (lo < n && kf[lo] == id) ? lo : -1;
}

// Rkfcur = Rkfw * Rwcur (:1082-1084, :489): both by Eigen's toRotationMatrix from the quaternions as held
__device__ __forceinline__ void fkf_rkfcur(const double *kf_Tcw, const double *cur_Twc, double R[9])
{
    double A[9], B[9];
    tri_rotmat(TriQ{kf_Tcw[3], kf_Tcw[4], kf_Tcw[5], kf_Tcw[6]}, A);
    tri_rotmat(TriQ{cur_Twc[3], cur_Twc[4], cur_Twc[5], cur_Twc[6]}, B);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) R[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
}

// cv::norm(projCamToImage(R bv) - kf_unpx), :514-517 / :1110-1117
__device__ __forceinline__ double fkf_unrot_dist(const double K[4], const double R[9], const double *bv, float2 kf_unpx)
{
    return tri_pdist(tri_project(K, tri_matvec(R, TriD3{bv[0], bv[1], bv[2]})), kf_unpx);
}

// :517 over the 64 distances a wavefront holds (lane l: term l of this trip, +0 where there is none): every lane adds them one after
// the other from lane 0 up (a broadcast per term), sum = (float)((double)sum + d)
__device__ __forceinline__ float fkf_wide_add64(float sum, double d)
{
    const int lo = __double2loint(d), hi = __double2hiint(d);
#pragma unroll
    for (int l = 0; l < 64; l++)
        sum = (float)((double)sum + __hiloint2double(__builtin_amdgcn_readlane(hi, l), __builtin_amdgcn_readlane(lo, l)));
    return sum;
}

// every input check fkf.hip makes on its items (full: the arrays the parallax / decision kernel reads); N / M: the keypoints of all
// frames / keyframes, n_max: the largest frame
int fkf_check_items(int n_items, const ov2_fkf_item *items, bool full, size_t *N, size_t *M, int *n_max);

// the kernels' parameter block, the item record and the result ints of fkf.hip: the lock-step step (mono.hip) fills the records on
// the device and reads the ints
struct FkfParamsD {
    double K[4];
    int ncellsize, nbwcells, nbhcells, nbmaxkps;
    float finit_parallax;
    int stereo, unrot, filter, stat, decide;
};
// 176 bytes, 16-byte aligned sections in the staging buffer
struct FkfItemD {
    int cur0, n_cur, kf0, n_kf;
    int cur_id, kf_id, kf_nb3dkps, localba_is_on;
    int noccupcells, nb3dkps, pad0, pad1;
    double cur_time, kf_time;
    double cur_Twc[7], kf_Tcw[7];
};
#define FKF_OUT_INTS 12       // per item: parallax bits, n, n_distinct, n_nonfinite, noccupcells, nb3dkps, n_out_of_grid, decision, reason

// what ov2_kf_decision refuses in its params (the grid)
int fkf_check_decide(const ov2_fkf_params *params);
// k_fkf_parallax in the form of ov2_kf_decision_batch on a caller-owned device block (fkf.hip)
int ov2_launch_kf_decision(hipStream_t s, const ov2_fkf_params *params, int n_items, const FkfItemD *items_d, const int *cur_lmid,
                           const float2 *cur_px, const float2 *cur_unpx, const double *cur_bv, const uint8_t *cur_is3d, const int *kf_lmid,
                           const float2 *kf_unpx, int *out_d);
// k_fkf_parallax in the form of ov2_parallax_batch(unrot, filter, stat) on a caller-owned device block (fkf.hip): out_d gets the
// parallax bits, n, n_distinct and n_nonfinite of every item
int ov2_launch_parallax(hipStream_t s, const ov2_fkf_params *params, int unrot, int filter, int stat, int n_items, const FkfItemD *items_d,
                        const int *cur_lmid, const float2 *cur_unpx, const double *cur_bv, const uint8_t *cur_is3d, const int *kf_lmid,
                        const float2 *kf_unpx, int *out_d);
