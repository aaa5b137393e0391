// createkf.hip -- the kernels of ov2_btracker_create_keyframe (trackb.hip), the lock-step form of MapManager::createKeyframe
// (src/map_manager.cpp:44-61, :286-362 of the reference) for the items of a batch that were asked to become keyframes:
//   k_ckf_prepare   noccupcells_ as Frame::addKeypointToGrid leaves it (the counting of k_fkf_parallax: Frame::getKeypointCellIdx, a
//                   bitmap of the cells in LDS) and nb3dkps_, nb2detect = nbmaxkps - noccupcells, and the detector's skip byte: an
//                   item that was not flagged, or needs no new point, costs the detection nothing.
//   k_ckf_append    addKeypointsToFrame (:322-341): the detector's points behind slot n_prev in its output order, lmid = nlmid_ + k,
//                   colour = level 0 at ((int)y, (int)x); more than n_max keypoints: OV2_CKF_OVERFLOW and nothing else.
//   k_ckf_install   addKeyframe as far as the tracker holds it: (lmid, slot) pairs sorted in LDS (bitonic, padded to a power of two),
//                   a repeated id found on the sorted keys (OV2_CKF_DUP_LMID, nothing written), else lmid / unpx / bv gathered into the
//                   arrays ov2_btracker_set_keyframe writes, the header {n_kf, Twc, Tcw = fe_invert_hd(Twc)} and the keyframe info.
// One work-group per item each; between them run the launches of detect.hip, keypoint.hip and brief.hip.  No scratch, vector stores only.
#include "createkf_dev.hpp"

#pragma clang fp contract(off)

#define CKF_THREADS 256

__global__ __launch_bounds__(CKF_THREADS) void k_ckf_prepare(CkfArgs a)
{
    __shared__ unsigned s_bm[OV2_FKF_MAX_CELLS / 32];
    __shared__ int s_cnt[2];                            // nb3dkps, noccupcells
    const int b = blockIdx.x, t = threadIdx.x;
    ov2_create_keyframe_result *rec = a.rec + b;
    if (!a.flag[b]) {                                   // (work-group uniform)
        if (t < 8) ((int *)rec)[t] = 0;                 // OV2_CKF_NOT_REQUESTED
        if (t == 0) { a.skip[b] = 1; a.nb[b] = 0; }
        return;
    }
    const int n = a.n[b], ncells = a.nbwcells * a.nbhcells, nwords = (ncells + 31) >> 5;
    for (int w = t; w < nwords; w += CKF_THREADS) s_bm[w] = 0u;
    if (t < 2) s_cnt[t] = 0;
    __syncthreads();
    const size_t o = (size_t)b * (size_t)a.n_max;
    int my_3d = 0;
    for (int i = t; i < n; i += CKF_THREADS) {
        my_3d += a.is3d[o + i] ? 1 : 0;
        const float2 px = a.px[o + i];                  // Frame::getKeypointCellIdx, frame.cpp:587-592
        const float rf = floorf(px.y / (float)a.ncellsize), cf = floorf(px.x / (float)a.ncellsize);
        bool inside = fabsf(rf) <= 1048576.f && fabsf(cf) <= 1048576.f;      // false for NaN too
        long long idx = 0;
        if (inside) {
            idx = (long long)(int)rf * a.nbwcells + (int)cf;
            inside = idx >= 0 && idx < ncells;
        }
        if (inside) atomicOr(&s_bm[idx >> 5], 1u << (idx & 31));
    }
    if (my_3d) atomicAdd(&s_cnt[0], my_3d);
    __syncthreads();
    int c = 0;
    for (int w = t; w < nwords; w += CKF_THREADS) c += __popc(s_bm[w]);
    if (c) atomicAdd(&s_cnt[1], c);
    __syncthreads();
    if (t != 0) return;
    const int nocc = s_cnt[1], nb2 = a.nbmaxkps - nocc;
    rec->action = OV2_CKF_CREATED;                      // until k_ckf_append / k_ckf_install find otherwise
    rec->n_prev = n; rec->noccupcells = nocc; rec->nb2detect = nb2; rec->n_new = 0; rec->n_kf = n; rec->nb3dkps = s_cnt[0]; rec->pad = 0;
    a.skip[b] = (a.det_on && nb2 > 0) ? 0 : 1;
    a.nb[b] = 0;
}

__global__ __launch_bounds__(CKF_THREADS) void k_ckf_append(CkfArgs a)
{
    const int b = blockIdx.x, t = threadIdx.x;
    if (!a.flag[b]) return;
    ov2_create_keyframe_result *rec = a.rec + b;
    const int n_prev = a.n[b], n_new = a.skip[b] ? 0 : a.so_n[(size_t)b * (size_t)a.so_stride];
    const bool over = n_new < 0 || n_new > a.det_cap || n_prev + n_new > a.n_max;
    if (!over) {
        const size_t o = (size_t)b * (size_t)a.n_max + (size_t)n_prev;
        const float2 *det = a.det + (size_t)b * (size_t)a.det_cap;
        const uint8_t *im = a.img + (long long)b * a.img_item;
        const int lm0 = a.nlmid[b];
        for (int k = t; k < n_new; k += CKF_THREADS) {
            const float2 p = det[k];
            a.px[o + k] = p;
            a.lmid[o + k] = lm0 + k;
            int x = (int)p.x, y = (int)p.y;             // im.at<uchar>(pt.y, pt.x): the C++ conversion truncates; a detected point lies in the image
            x = x < 0 ? 0 : (x > a.w - 1 ? a.w - 1 : x); y = y < 0 ? 0 : (y > a.h - 1 ? a.h - 1 : y);
            a.color[o + k] = im[(long long)y * a.img_pitch + x];
        }
    }
    if (t != 0) return;
    rec->n_new = n_new;
    rec->n_kf = n_prev + n_new;
    if (over) rec->action = OV2_CKF_OVERFLOW;
    a.nb[b] = over ? 0 : n_prev + n_new;
}

__global__ __launch_bounds__(CKF_THREADS) void k_ckf_install(CkfArgs a)
{
    __shared__ unsigned long long s_key[OV2_FKF_MAX_POINTS];      // lmid << 32 | slot; the padding sorts behind every id
    __shared__ int s_dup;
    const int b = blockIdx.x, t = threadIdx.x;
    if (!a.flag[b]) return;
    ov2_create_keyframe_result *rec = a.rec + b;
    if (rec->action != OV2_CKF_CREATED) return;         // (work-group uniform: written by the launch before this one)
    const int n_kf = a.nb[b];
    const size_t o = (size_t)b * (size_t)a.n_max;
    int np = 2;
    while (np < n_kf) np <<= 1;                          // n_kf <= n_max <= OV2_FKF_MAX_POINTS, checked by the host
    for (int i = t; i < np; i += CKF_THREADS)
        s_key[i] = i < n_kf ? (((unsigned long long)(unsigned)a.lmid[o + i] << 32) | (unsigned)i) : ~0ull;      // ids are >= 0 (the host checked)
    if (t == 0) s_dup = 0;
    for (int k = 2; k <= np; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int x = t; x < (np >> 1); x += CKF_THREADS) {
                const int i = ((x & ~(j - 1)) << 1) | (x & (j - 1)), l = i | j;
                const unsigned long long u = s_key[i], v = s_key[l];
                if ((u > v) == ((i & k) == 0)) { s_key[i] = v; s_key[l] = u; }
            }
        }
    __syncthreads();
    bool dup = false;
    for (int i = t; i + 1 < n_kf; i += CKF_THREADS) dup = dup || (unsigned)(s_key[i] >> 32) == (unsigned)(s_key[i + 1] >> 32);
    if (dup) s_dup = 1;
    __syncthreads();
    if (s_dup) {
        if (t == 0) rec->action = OV2_CKF_DUP_LMID;
        return;
    }
    for (int i = t; i < n_kf; i += CKF_THREADS) {
        const unsigned long long key = s_key[i];
        const int slot = (int)(unsigned)(key & 0xffffffffull);
        a.kf_lmid[o + i] = (int)(unsigned)(key >> 32);
        a.kf_unpx[o + i] = a.unpx[o + slot];
        const double *bv = a.bv + 3 * (o + slot);
        double *kb = a.kf_bv + 3 * (o + i);
        kb[0] = bv[0]; kb[1] = bv[1]; kb[2] = bv[2];
        a.perm[o + i] = slot;
    }
    if (t != 0) return;
    FeKfHdr h;
    h.n_kf = n_kf; h.pad = 0;
    const double *T = a.Twc + 7 * (size_t)b;
    for (int c = 0; c < 7; c++) h.kf_Twc[c] = T[c];
    fe_invert_hd(h.kf_Twc, h.kf_Tcw);
    a.hdr[b] = h;
    a.o_hdr[b] = h;
    a.r_ki[b] = MonoKfInfo{a.nkfid[b], rec->nb3dkps, 1, 0};
    a.r_kt[b] = a.time[b];
}

int ov2_launch_ckf_prepare(hipStream_t s, const CkfArgs &a, int n_active)
{
    hipLaunchKernelGGL(k_ckf_prepare, dim3(n_active), dim3(CKF_THREADS), 0, s, a);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

int ov2_launch_ckf_append(hipStream_t s, const CkfArgs &a, int n_active)
{
    hipLaunchKernelGGL(k_ckf_append, dim3(n_active), dim3(CKF_THREADS), 0, s, a);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

int ov2_launch_ckf_install(hipStream_t s, const CkfArgs &a, int n_active)
{
    hipLaunchKernelGGL(k_ckf_install, dim3(n_active), dim3(CKF_THREADS), 0, s, a);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}
