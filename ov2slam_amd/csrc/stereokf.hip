// stereokf.hip -- the kernels of ov2_btracker_stereo_keyframe (f22; trackb.hip) around the existing ones: the mapper's stereo block
// on the resident keyframe (MapManager::stereoMatching, src/map_manager.cpp:367-611, then Mapper::triangulateStereo,
// src/mapper.cpp:346-461) without leaving the device.  The item is the grid axis, 256 threads, no scratch, no atomics.
//   k_skf_input      ONE WORK-GROUP PER ITEM.  The resident frame into the ranges k_prior_stereo, k_track_klt, k_epipolar_check and
//                    k_triangulate read: px, state = is3d, the point, unpx / bv by the left camera (the arithmetic of
//                    k_compute_keypoints), the keypoint on the coarsest level, src = -1; the keyframe's Twc / Tcw out of its header;
//                    the per-item descriptors (count 0 where the item is not OV2_SKF_DONE).  Without rectification the keypoint
//                    grid of Frame::getSurroundingKeypoints: the cell of every keypoint in LDS, then a keypoint's place in cell_kp
//                    is the number of keypoints in a lower cell plus those of its own cell in a lower slot -- KEYPOINTS OF A CELL
//                    STAND IN SLOT ORDER -- and cell_start[c], a lane per cell, is the number of keypoints in a lower cell.  Both
//                    are counts over the LDS table (every lane reads the same entry: a broadcast): no order of lanes or wavefronts
//                    enters.
//   k_skf_seed       one thread per slot behind k_prior_stereo: flag = has_prior != 0 (k_track_klt reads bit 0, and a neighbour
//                    prior is kind 2); without rectification the line search's "nothing found", the bytes of the host route's fill.
//   k_skf_stereo_kp  one thread per slot behind k_epipolar_check: stereo_ok = tracked && gate, right_px ((0, 0) where the tracking
//                    failed), runpx / rbv of the stereo_ok slots by the right camera, is_stereo = stereo_ok && !is3d.
//   k_skf_apply      ONE WORK-GROUP PER ITEM behind k_triangulate: the frame with is3d = 1 and the new point on every
//                    OV2_TRI_STEREO_OK slot into the item's OTHER buffer, the record's counts (a ballot per wavefront, the
//                    wavefronts' sums in LDS), kf_nb3dkps of the resident keyframe info.
// Every count read from device memory is clamped against n_max before it indexes anything.
#include "stereokf_dev.hpp"

#pragma clang fp contract(off)

static_assert(sizeof(ov2_stereo_keyframe_result) == 32, "stereo keyframe record");

// Frame::computeKeypoint (frame.cpp:246-254) as k_compute_keypoints (keypoint.hip) computes it
__device__ __forceinline__ float2 skf_compute_keypoint(const KpCalib &c, float2 p, double b[3])
{
    const float2 u = kp_undistort_image_point(c, p);
    const double x = (double)u.x, y = (double)u.y;
#pragma unroll
    for (int r = 0; r < 3; r++) b[r] = (c.iK[3 * r] * x + c.iK[3 * r + 1] * y) + c.iK[3 * r + 2] * 1.;
    const double nrm = sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
    b[0] = b[0] / nrm; b[1] = b[1] / nrm; b[2] = b[2] / nrm;
    return u;
}

__global__ __launch_bounds__(SKF_THREADS) void k_skf_input(SkfArgs a)
{
    __shared__ int s_cell[OV2_FKF_MAX_POINTS];
    const int b = blockIdx.x, t = threadIdx.x;
    const int nm = a.n_max < OV2_FKF_MAX_POINTS ? a.n_max : OV2_FKF_MAX_POINTS;
    const int ncells = a.rect ? 0 : a.nbw * a.nbh;
    const size_t o = (size_t)b * (size_t)a.n_max;
    const bool on = a.act[b] != 0;
    int n = 0;
    ResItem src = ResItem();
    if (on) { src = res_item(a.f, b, 0); n = res_clamp(*src.n, nm); }
    if (t == 0) {
        a.pit[b] = SkfItemD{(int)o, n, b * (ncells + 1), (int)o};
        a.tit[b] = make_int4((int)o, n, 0, 0);
        a.nd[b] = n;
    }
    if (!on) return;
    if (t < 7) { a.Tcw[7 * (size_t)b + t] = a.hdr[b].kf_Tcw[t]; a.Twc[7 * (size_t)b + t] = a.hdr[b].kf_Twc[t]; }
    for (int i = t; i < n; i += SKF_THREADS) {
        const size_t s = o + (size_t)i;
        const float2 p = src.px[i];
        double bv[3];
        const float2 u = skf_compute_keypoint(a.left, p, bv);
        a.px[s] = p;
        a.unpx[s] = u;
        a.bv[3 * s] = bv[0]; a.bv[3 * s + 1] = bv[1]; a.bv[3 * s + 2] = bv[2];
        a.state[s] = (uint8_t)(src.is3d[i] != 0);
        a.fw[3 * s] = src.wpt[3 * i]; a.fw[3 * s + 1] = src.wpt[3 * i + 1]; a.fw[3 * s + 2] = src.wpt[3 * i + 2];
        a.top[s] = make_float2(p.x * a.down, p.y * a.down);                     // map_manager.cpp:427
        a.src[s] = -1;
        if (!a.rect) {
            const float rf = floorf(p.y / a.cellsize), cf = floorf(p.x / a.cellsize);   // frame.cpp:599-600, as k_prior_stereo
            const bool in = rf >= 0.f && cf >= 0.f && rf < (float)a.nbh && cf < (float)a.nbw;   // false for NaN
            s_cell[i] = in ? (int)rf * a.nbw + (int)cf : -1;
        }
    }
    if (a.rect) return;
    __syncthreads();
    int *ck = a.cell_kp + o;
    for (int i = t; i < n; i += SKF_THREADS) {
        const int c = s_cell[i];
        if (c < 0) continue;
        int pos = 0;
        for (int j = 0; j < n; j++) {
            const int cj = s_cell[j];
            pos += (cj >= 0 && (cj < c || (cj == c && j < i))) ? 1 : 0;
        }
        ck[pos] = i;                                                             // pos < the keypoints inside the grid <= n
    }
    int *cs = a.cell_start + (size_t)b * (size_t)(ncells + 1);
    for (int c = t; c <= ncells; c += SKF_THREADS) {
        int cnt = 0;
        for (int j = 0; j < n; j++) {
            const int cj = s_cell[j];
            cnt += (cj >= 0 && cj < c) ? 1 : 0;
        }
        cs[c] = cnt;
    }
}

__global__ __launch_bounds__(SKF_THREADS) void k_skf_seed(SkfArgs a)
{
    const int b = blockIdx.y, i = blockIdx.x * SKF_THREADS + threadIdx.x;
    if (i >= res_clamp(a.nd[b], a.n_max)) return;
    const size_t s = (size_t)b * (size_t)a.n_max + (size_t)i;
    a.flag[s] = a.has_prior[s] != 0 ? 1 : 0;
    if (!a.rect) a.sadx[s] = __int_as_float((int)0xBFBFBFBFu);                  // < 0: nothing found (stereo.hip: the 0xBF fill)
}

__global__ __launch_bounds__(SKF_THREADS) void k_skf_stereo_kp(SkfArgs a)
{
    const int b = blockIdx.y, i = blockIdx.x * SKF_THREADS + threadIdx.x;
    if (i >= res_clamp(a.nd[b], a.n_max)) return;
    const size_t s = (size_t)b * (size_t)a.n_max + (size_t)i;
    const bool tracked = (a.lk_st[s] & 1) != 0, ok = tracked && a.gate_ok[s] != 0;
    const float2 rp = tracked ? a.lk_out[s] : make_float2(0.f, 0.f);
    a.right_px[s] = rp;
    a.stereo_ok[s] = ok ? 1 : 0;
    float2 ru = make_float2(0.f, 0.f);
    double bv[3] = {0., 0., 0.};
    if (ok) ru = skf_compute_keypoint(a.right, rp, bv);                          // Frame::computeStereoKeypoint, frame.cpp:405-420
    a.runpx[s] = ru;
    a.rbv[3 * s] = bv[0]; a.rbv[3 * s + 1] = bv[1]; a.rbv[3 * s + 2] = bv[2];
    a.is_stereo[s] = (ok && a.state[s] == 0) ? 1 : 0;                            // mapper.cpp:383
}

__global__ __launch_bounds__(SKF_THREADS) void k_skf_apply(SkfArgs a)
{
    __shared__ int s_tot[SKF_WAVES][6];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (!a.act[b]) return;
    const int nm = a.n_max < OV2_FKF_MAX_POINTS ? a.n_max : OV2_FKF_MAX_POINTS;
    const size_t o = (size_t)b * (size_t)a.n_max;
    const ResItem src = res_item(a.f, b, 0), dst = res_item(a.f, b, 1);
    const int n = res_clamp(*src.n, nm);
    int c_p1 = 0, c_p2 = 0, c_sok = 0, c_tried = 0, c_good = 0, c_3d = 0;
    for (int i0 = 0; i0 < n; i0 += SKF_THREADS) {
        const int i = i0 + t;
        const bool in = i < n;
        int hp = 0, st = 0; bool sok = false, d3 = false;
        if (in) {
            const size_t s = o + (size_t)i;
            hp = a.has_prior[s]; st = a.tri_status[s]; sok = a.stereo_ok[s] != 0;
            const bool good = (st & OV2_TRI_STEREO_OK) != 0;
            d3 = good || src.is3d[i] != 0;
            dst.px[i] = src.px[i];
            dst.lmid[i] = src.lmid[i];
            dst.is3d[i] = d3 ? 1 : 0;
            dst.wpt[3 * i] = good ? a.tri_wpt[3 * s] : src.wpt[3 * i];
            dst.wpt[3 * i + 1] = good ? a.tri_wpt[3 * s + 1] : src.wpt[3 * i + 1];
            dst.wpt[3 * i + 2] = good ? a.tri_wpt[3 * s + 2] : src.wpt[3 * i + 2];
        }
        c_p1 += __popcll(__ballot(in && hp == 1)); c_p2 += __popcll(__ballot(in && hp == 2)); c_sok += __popcll(__ballot(in && sok));
        c_tried += __popcll(__ballot(in && (st & OV2_TRI_STEREO_TRIED) != 0)); c_good += __popcll(__ballot(in && (st & OV2_TRI_STEREO_OK) != 0));
        c_3d += __popcll(__ballot(in && d3));
    }
    if (lane == 0) { s_tot[wave][0] = c_p1; s_tot[wave][1] = c_p2; s_tot[wave][2] = c_sok; s_tot[wave][3] = c_tried; s_tot[wave][4] = c_good; s_tot[wave][5] = c_3d; }
    __syncthreads();
    if (t != 0) return;
    int v[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int w = 0; w < SKF_WAVES; w++)
#pragma unroll
        for (int k = 0; k < 6; k++) v[k] += s_tot[w][k];
    *dst.n = n;
    ov2_stereo_keyframe_result r;
    r.action = OV2_SKF_DONE; r.n = n; r.n_prior3d = v[0]; r.n_prior_nb = v[1]; r.n_stereo_kps = v[2]; r.n_stereo = v[3]; r.n_stereo_good = v[4];
    r.nb3dkps = v[5];
    a.rec[b] = r;
    a.r_ki[b].kf_nb3dkps = v[5];                                                 // updateMapPoint -> turnKeypoint3d on the keyframe
}

int ov2_launch_skf_input(hipStream_t s, const SkfArgs &a, int n_active)
{
    hipLaunchKernelGGL(k_skf_input, dim3(n_active), dim3(SKF_THREADS), 0, s, a);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

int ov2_launch_skf_seed(hipStream_t s, const SkfArgs &a, int n_active)
{
    hipLaunchKernelGGL(k_skf_seed, dim3((a.n_max + SKF_THREADS - 1) / SKF_THREADS, n_active), dim3(SKF_THREADS), 0, s, a);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

int ov2_launch_skf_stereo_kp(hipStream_t s, const SkfArgs &a, int n_active)
{
    hipLaunchKernelGGL(k_skf_stereo_kp, dim3((a.n_max + SKF_THREADS - 1) / SKF_THREADS, n_active), dim3(SKF_THREADS), 0, s, a);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

int ov2_launch_skf_apply(hipStream_t s, const SkfArgs &a, int n_active)
{
    hipLaunchKernelGGL(k_skf_apply, dim3(n_active), dim3(SKF_THREADS), 0, s, a);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}
