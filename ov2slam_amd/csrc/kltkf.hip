// kltkf.hip -- the from-keyframe mode of the lock-step tracker (VisualFrontEnd::kltTrackingFromKF, src/visual_front_end.cpp:278-442;
// trackb.hip: ov2_btracker_set_track_from_keyframe): what surrounds the tracking kernels k_track_klt_kf_w / k_track_klt_kf (lkw.hip,
// lk.hip).  The reference tracks every frame from kf_pyr_, a copy of the current pyramid taken when the keyframe was created
// (:52-54), and from the keyframe's px_ of every lmid_ (:336, :346); a keypoint whose lmid_ the keyframe no longer holds leaves the
// frame before anything is tracked (:316-320, :348-351).
//   k_kfpyr_adopt    the copy of :52-54 for every flagged item in one launch: a pure streaming copy of the whole item stride (every
//                    level with its borders), 16 bytes per lane, grid (chunk, item); an unflagged item costs its blocks one byte read
//   k_kfpx_install   the keyframe's px_ by ascending lmid_ (the px table), from the create-keyframe block
//   k_kf_join        per slot of the frame: membership by binary search in the resident keyframe's ids, the source point by binary
//                    search in the px table; k_prior_frame's prior stays (the projection where its flag is set, else the frame's own
//                    px: :343-345), a slot outside the keyframe gets flag 2 (no prior, skipped)
// and the host's half of the 33 % rule (:395-400).
#include "kltkf_dev.hpp"
#include "keypoint_dev.hpp"
#include <algorithm>
#include <vector>

#define KFA_THREADS 256
#define KFA_UNROLL 4                                    // 16-byte words in flight per lane
#define KFJ_THREADS 256

__global__ __launch_bounds__(KFA_THREADS) void k_kfpyr_adopt(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, long long src_stride,
                                                             long long dst_stride, unsigned words, const uint8_t *__restrict__ flag)
{
    const int item = blockIdx.y;
    if (!flag[item]) return;                            // block-uniform
    const uint4 *s = (const uint4 *)(src + (long long)item * src_stride);
    uint4 *d = (uint4 *)(dst + (long long)item * dst_stride);
    const unsigned step = gridDim.x * (KFA_THREADS * KFA_UNROLL);
    for (unsigned w0 = blockIdx.x * (KFA_THREADS * KFA_UNROLL) + threadIdx.x; w0 < words; w0 += step) {
        uint4 v[KFA_UNROLL];
#pragma unroll
        for (int k = 0; k < KFA_UNROLL; k++) {
            const unsigned w = w0 + k * KFA_THREADS;
            if (w < words) v[k] = s[w];
        }
#pragma unroll
        for (int k = 0; k < KFA_UNROLL; k++) {
            const unsigned w = w0 + k * KFA_THREADS;
            if (w < words) d[w] = v[k];
        }
    }
}

__global__ __launch_bounds__(KFJ_THREADS) void k_kfpx_install(KfPxInstallArgs a)
{
    const int b = blockIdx.x, t = threadIdx.x;
    const bool on = a.make_kf[b] != 0 && a.rec[b].action == OV2_CKF_CREATED;    // (written by the launches before this one)
    if (t == 0) a.adopt[b] = on ? 1 : 0;
    if (!on) return;
    int n = a.rec[b].n_kf;
    n = n < 0 ? 0 : (n > a.tab.n_max ? a.tab.n_max : n);
    uint8_t *it = a.tab.base + (size_t)b * a.tab.k_item;
    int *lm = (int *)(it + a.tab.k_lm);
    float2 *px = (float2 *)(it + a.tab.k_px);
    const size_t o = (size_t)b * (size_t)a.tab.n_max;
    for (int i = t; i < n; i += KFJ_THREADS) {
        const int slot = a.perm[o + i];
        lm[i] = a.lmid[o + slot];
        px[i] = a.px[o + slot];
    }
    if (t == 0) *(int *)it = n;
}

// index of `key` in the ascending list v[0, n), or -1
__device__ __forceinline__ int kf_find(const int *__restrict__ v, int n, int key)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (v[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo < n && v[lo] == key ? lo : -1;
}

// Behind k_prior_frame (priors.hip), which has written prior = the projection and flag 1 where there is one, else prior = the frame's
// own px and flag 0: that IS kltTrackingFromKF's prior (:326-345), so only the source point and the skip flag are written here.  The
// retry prior (:386) is the frame's px too: the step hands the tracking kernel its keypoint array for it.
__global__ __launch_bounds__(KFJ_THREADS) void k_kf_join(KfJoinArgs a)
{
    const int b = blockIdx.x;
    const int nm = a.tab.n_max;
    int n = a.n_dev[b];
    n = n < 0 ? 0 : (n > nm ? nm : n);
    int n_kf = a.hdr[b].n_kf;
    n_kf = n_kf < 0 ? 0 : (n_kf > nm ? nm : n_kf);
    const uint8_t *it = a.tab.base + (size_t)b * a.tab.k_item;
    int n_tab = *(const int *)it;
    n_tab = n_tab < 0 ? 0 : (n_tab > nm ? nm : n_tab);
    const int *tab_lm = (const int *)(it + a.tab.k_lm);
    const float2 *tab_px = (const float2 *)(it + a.tab.k_px);
    const size_t o = (size_t)b * (size_t)nm;
    for (int i = threadIdx.x; i < n; i += KFJ_THREADS) {
        const int lm = a.lmid[o + i];
        const int j = kf_find(a.kf_lmid + o, n_kf, lm) >= 0 ? kf_find(tab_lm, n_tab, lm) : -1;
        if (j >= 0) a.src[o + i] = tab_px[j];
        else { a.src[o + i] = a.kps[o + i]; a.flags[o + i] = 2; }
    }
}

int ov2_launch_kfpx_install(hipStream_t s, const KfPxInstallArgs &a, int n_active)
{
    hipLaunchKernelGGL(k_kfpx_install, dim3(n_active), dim3(KFJ_THREADS), 0, s, a);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

int ov2_launch_kfpyr_adopt(hipStream_t s, const PyrDesc &cur, const PyrDesc &store, const uint8_t *flag_d, int n_active)
{
    OV2_REQUIRE(cur.item_stride == store.item_stride && cur.item_stride % 16 == 0 && cur.item_stride / 16 <= 0x7fffffffll, OV2_EINVAL,
                "the keyframe store and the tracker's pyramids differ in geometry");
    OV2_REQUIRE(n_active >= 1 && n_active <= cur.batch && n_active <= store.batch && n_active <= 65535, OV2_EINVAL, "n_active out of range");
    const unsigned words = (unsigned)(cur.item_stride / 16);
    const unsigned per_block = KFA_THREADS * KFA_UNROLL;
    unsigned chunks = (words + per_block - 1) / per_block;
    // a memory-bound launch: about 2048 work-groups in all, each striding over its item's chunks
    const unsigned cap = 2048u / (unsigned)n_active > 0 ? 2048u / (unsigned)n_active : 1u;
    if (chunks > cap) chunks = cap;
    hipLaunchKernelGGL(k_kfpyr_adopt, dim3(chunks, n_active), dim3(KFA_THREADS), 0, s, (const uint8_t *)cur.base, store.base,
                       cur.item_stride, store.item_stride, words, flag_d);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

int ov2_launch_kf_join(hipStream_t s, const KfJoinArgs &a, int n_active)
{
    hipLaunchKernelGGL(k_kf_join, dim3(n_active), dim3(KFJ_THREADS), 0, s, a);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

int ov2_apply_p3p_rule_kf(ov2_ctx *ctx, const ov2_tracker_config &c, const ov2_pyr *kf, const ov2_pyr *cur, const KpCalib *calib,
                          const KfRuleFrame &f, int *p3p_req)
{
    const int n = f.n;
    size_t nbkps = 0, nbgood = 0;
    for (int i = 0; i < n; i++) if (f.flags[i] & 1) { nbkps++; if ((f.status[i] & 3) == 1) nbgood++; }
    int p3p = 0;
    if (nbkps > 0 && (double)nbgood < 0.33 * (double)nbkps) {
        p3p = 1;
        std::vector<int> idx;
        for (int i = 0; i < n; i++) if (!(f.flags[i] & 2) && (!(f.flags[i] & 1) || (f.status[i] & 2))) idx.push_back(i);
        if (!idx.empty()) {
            const int m = (int)idx.size();
            std::vector<float> k2(2 * (size_t)m), p2(2 * (size_t)m);
            std::vector<uint8_t> s2((size_t)m);
            for (int j = 0; j < m; j++) {
                // (k_kf_join found the id in the table: a slot that it did not carries flag 2)
                const int *e = std::lower_bound(f.tab_lmid, f.tab_lmid + f.n_tab, f.lmid[idx[j]]);
                OV2_REQUIRE(e != f.tab_lmid + f.n_tab && *e == f.lmid[idx[j]], OV2_EINVAL, "the keyframe-px table's host mirror and the device disagree");
                const float *q = f.tab_px + 2 * (e - f.tab_lmid);
                k2[2 * j] = p2[2 * j] = q[0]; k2[2 * j + 1] = p2[2 * j + 1] = q[1];
            }
            const int rc = ov2_fb_klt(ctx, kf, cur, c.win, c.nklt_pyr_lvl, c.max_iter, c.eps, c.err_th, c.fb_dist, k2.data(), p2.data(), m,
                                      s2.data(), nullptr);
            if (rc != OV2_OK) return rc;
            for (int j = 0; j < m; j++) {
                f.out_xy[2 * idx[j]] = p2[2 * j]; f.out_xy[2 * idx[j] + 1] = p2[2 * j + 1];
                f.status[idx[j]] = (uint8_t)((f.status[idx[j]] & 2) | (s2[j] ? 1 : 0));
            }
            if (calib) {                                               // their undistorted pixels / bearings follow the new positions
                std::vector<float> u2(2 * (size_t)m);
                std::vector<double> b2(3 * (size_t)m);
                const KpCalib &kc = *calib;
                const double Kk[4] = {kc.fx, kc.fy, kc.cx, kc.cy};
                const int rck = ov2_compute_keypoints(ctx, kc.model, Kk, kc.nD ? kc.k : nullptr, kc.nD, kc.iK, p2.data(), m, u2.data(), b2.data());
                if (rck != OV2_OK) return rck;
                for (int j = 0; j < m; j++) {
                    memcpy(f.unpx + 2 * (size_t)idx[j], &u2[2 * (size_t)j], 8);
                    memcpy(f.bv + 3 * (size_t)idx[j], &b2[3 * (size_t)j], 24);
                }
            }
        }
    }
    if (p3p_req) *p3p_req = p3p;
    return OV2_OK;
}
