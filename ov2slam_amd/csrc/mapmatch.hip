// mapmatch.hip -- local-map matching for gfx950, in the reference's two forms: Mapper::matchToMap (src/mapper.cpp:576-774,
// ov2_match_to_map*) and LoopCloser::matchToMap (src/loop_closer.cpp:586-763, ov2_loop_match_to_map*, which
// LoopCloser::trackLoopLocalMap runs after P3P has put the new keyframe into the loop keyframe's frame).
//   k_map_match<LOOP>  ONE WAVEFRONT PER LOCAL MAP POINT: project it into the keyframe with the pose the caller passes (fp64,
//                  wave-uniform gates), put a lane on each keypoint of the 2x2 block of cells around the projection for the gates
//                  that need no other map point (usable map point, pixel distance), then walk the survivors in the reference's
//                  order and spread each one's inner work over the lanes: shared-observer test (a lane per observation of the
//                  candidate, binary search in the point's sorted ids, one ballot), re-projection into the candidate's observing
//                  keyframes (a lane per observation, then the float sum in ascending keyframe id, lane by lane), minimum Hamming
//                  distance (a lane per descriptor pair, wave minimum).  The point's proposal goes into its keypoint's key with a
//                  64-bit atomic minimum on (distance << 32 | reversed local-map index): smallest distance, among equals the point
//                  listed last, whatever the order the wavefronts retire in.
//                  LOOP = true (the loop closer) adds the matched-keypoint exclusion to the lane-local gates and has no
//                  re-projection into the candidate's observers -- so no pose table and no observer pixels.  The host differs in
//                  the viewing cone (the loop closer's is the reference's multiplied one) and in the pixel radius (the mapper
//                  doubles it for a keyframe with few 3-D keypoints; the loop closer takes it as given).
//   k_map_pick     one lane per keypoint: key -> (kp_lm, kp_dist).
// The point's own observation ids and descriptors are read through the vector cache where a candidate needs them: a point sees
// about one candidate that survives the pixel gate, so a staged copy would be written once and read once (DESIGN.md 4.16 has the
// loop closer's survivor count).  Poses as held, Sophus' SE3 * point, sums of three products in serial order, cv::norm of a
// Point2f difference: mvg_dev.hpp.  tests/match_ref.py and tests/loopmap_ref.py are the same arithmetic in numpy.  Every index the
// caller passes is validated on the host before the launch.
#include "common.hpp"
#include "keypoint_dev.hpp"
#include "mvg_dev.hpp"
#include <cmath>
#include <type_traits>

#pragma clang fp contract(off)

#define MT_WAVES 4
#define MT_BLOCK (64 * MT_WAVES)

static_assert(OV2_LOOPMAP_BEHIND == OV2_MATCH_BEHIND && OV2_LOOPMAP_OUT_OF_FOV == OV2_MATCH_OUT_OF_FOV &&
              OV2_LOOPMAP_OUT_OF_IMAGE == OV2_MATCH_OUT_OF_IMAGE && OV2_LOOPMAP_NO_CANDIDATE == OV2_MATCH_NO_CANDIDATE &&
              OV2_LOOPMAP_RATIO_REJECTED == OV2_MATCH_RATIO_REJECTED && OV2_LOOPMAP_BEST == OV2_MATCH_BEST,
              "the kernel writes one set of status bits for both call families");

// One batch item.  The per-item tables are concatenated over the batch; these are the item's first rows.  obs_start / desc_start /
// cell_start keep the caller's item-relative offsets (n_mp + 1 / ncells + 1 entries per item).
struct MapMatchItem {
    double Tcw[7];
    float dmax;                  // dmaxpxdist: fmax_proj_pxdist; the mapper doubles it when nb3dkps < 30
    int n_lm;
    int kp0, cell0, ck0, mp0;    // keypoints, cell_start, cell_kp, obs_start / desc_start
    int ob0, de0, kf0, lm0;      // observations, descriptors, poses (mapper only, else 0), local map points
};

// kp_matched: loop closer only.  obs_kf, obs_px, kf_Tcw: mapper only.  The other mode leaves them null and never reads them.
// kp_matched is last: between the other pointers it moves the mapper's arguments and costs that instantiation four more SGPR
// spills to VGPR lanes (compiled both ways).
struct MapMatchArgs {
    KpCalib cal;
    double img_w, img_h;
    float view_th, mindist, cellsize;
    int nbw;
    const MapMatchItem *items;
    const float2 *kp_px; const int *kp_mp; const int *cell_start; const int *cell_kp;
    const int *obs_start; const int *obs_kfid; const int *obs_kf; const float2 *obs_px;
    const int *desc_start; const uint4 *desc;
    const double *kf_Tcw; const int *lm_mp; const double *lm_wpt;
    uint8_t *lm_status; int *lm_kp; float *lm_dist; float2 *lm_projpx;
    unsigned long long *keys;
    const uint8_t *kp_matched;
};

// The reference lines in the comments: mapper.cpp / loop_closer.cpp.
template <bool LOOP>
__global__ __launch_bounds__(MT_BLOCK) void k_map_match(MapMatchArgs a)
{
    const MapMatchItem &it = a.items[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const int l = blockIdx.x * MT_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (l >= it.n_lm) return;
    const int gl = it.lm0 + l;
    const TriD3 w{a.lm_wpt[3 * (size_t)gl], a.lm_wpt[3 * (size_t)gl + 1], a.lm_wpt[3 * (size_t)gl + 2]};
    const TriD3 cp = tri_act(tri_load(it.Tcw), w);                   // frame.projWorldToCam, :628 / Tcw * wpt, :634
    int st = 0, bestid = -1, secid = -1;
    float2 ppx = make_float2(0.f, 0.f);
    float bestdist = 0.f, secdist = 0.f;
    if (cp.z < 0.1) {
        st = OV2_MATCH_BEHIND;
    } else if (fabsf((float)(cp.z / sqrt((cp.x * cp.x + cp.y * cp.y) + cp.z * cp.z))) < a.view_th) {   // :634-638 / :640-644
        st = OV2_MATCH_OUT_OF_FOV;
    } else {
        ppx = kp_project_dist(a.cal, cp.x, cp.y, cp.z);
        if (!(ppx.x >= 0 && ppx.y >= 0 && (double)ppx.x < a.img_w && (double)ppx.y < a.img_h)) st = OV2_MATCH_OUT_OF_IMAGE;   // isInImage
    }
    if (st == 0) {
        bestdist = secdist = a.mindist;
        const int rkp = __builtin_amdgcn_readfirstlane((int)floorf(ppx.y / a.cellsize));     // getSurroundingKeypoints, frame.cpp:624-650
        const int ckp = __builtin_amdgcn_readfirstlane((int)floorf(ppx.x / a.cellsize));
        const int A = it.mp0 + a.lm_mp[gl];
        const int oA = it.ob0 + a.obs_start[A], nA = a.obs_start[A + 1] - a.obs_start[A];
        const int dA = it.de0 + a.desc_start[A], nDA = a.desc_start[A + 1] - a.desc_start[A];
        // The block's keypoints in the reference's order: cells (rkp-1, ckp-1), (rkp-1, ckp), (rkp, ckp-1), (rkp, ckp), inside a
        // cell the order of cell_kp.  A lane per keypoint evaluates the gates that need no other map point (:663-669, :683 /
        // :672-685, :690-695); the survivors -- well under one per point on average -- are then handled one at a time in that order.
        int cs[4], cn[4], ncand = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int r = rkp - 1 + (q >> 1), c = ckp - 1 + (q & 1);
            cs[q] = cn[q] = 0;
            if (r >= 0 && c >= 0) {
                const int idx = it.cell0 + r * a.nbw + c;
                cs[q] = __builtin_amdgcn_readfirstlane(a.cell_start[idx]);
                cn[q] = __builtin_amdgcn_readfirstlane(a.cell_start[idx + 1]) - cs[q];
            }
            ncand += cn[q];
        }
        for (int q0 = 0; q0 < ncand; q0 += 64) {
            int kq = -1;
            bool pass = false;
            if (q0 + lane < ncand) {
                int t = q0 + lane, off = cs[0];
                if (t >= cn[0]) { t -= cn[0]; off = cs[1]; if (t >= cn[1]) { t -= cn[1]; off = cs[2]; if (t >= cn[2]) { t -= cn[2]; off = cs[3]; } } }
                kq = a.cell_kp[it.ck0 + off + t];
                const int Bq = a.kp_mp[it.kp0 + kq];
                bool taken = false;
                if constexpr (LOOP) taken = a.kp_matched[it.kp0 + kq] != 0;                  // lmid_ in vmatchedkpids, - / :672-675
                if (!taken && Bq >= 0 && a.desc_start[it.mp0 + Bq + 1] != a.desc_start[it.mp0 + Bq])   // kp.lmid_ >= 0, desc_ not empty
                    pass = !((float)tri_pdist(ppx, a.kp_px[it.kp0 + kq]) > it.dmax);         // :667-671 / :681-685
            }
            for (unsigned long long cand = __ballot(pass); cand; cand &= cand - 1) {
                const int k = __shfl(kq, __ffsll((long long)cand) - 1);
                const int B = it.mp0 + __builtin_amdgcn_readfirstlane(a.kp_mp[it.kp0 + k]);
                const int nDB = __builtin_amdgcn_readfirstlane(a.desc_start[B + 1] - a.desc_start[B]);
                const int oB = it.ob0 + a.obs_start[B];
                const int nB = __builtin_amdgcn_readfirstlane(a.obs_start[B + 1] - a.obs_start[B]);
                bool shared = false;                                                 // :686-696 / :697-707
                for (int j0 = 0; j0 < nB && !shared; j0 += 64) {
                    bool hit = false;
                    if (j0 + lane < nB) {
                        const int id = a.obs_kfid[oB + j0 + lane];
                        int lo = 0, hi = nA;
                        while (lo < hi) {
                            const int mid = (lo + hi) >> 1;
                            if (a.obs_kfid[oA + mid] < id) lo = mid + 1; else hi = mid;
                        }
                        hit = lo < nA && a.obs_kfid[oA + lo] == id;
                    }
                    shared = __ballot(hit) != 0ull;
                }
                if (shared) continue;
                if constexpr (!LOOP) {                                               // :698-714 / the loop closer has none
                    float coprojpx = 0.f;
                    unsigned nbcokp = 0;
                    for (int j0 = 0; j0 < nB; j0 += 64) {
                        double d = 0.;
                        bool valid = false;
                        const int j = j0 + lane;
                        if (j < nB) {
                            const int kf = a.obs_kf[oB + j];
                            if (kf >= 0) {
                                valid = true;
                                const TriD3 cc = tri_act(tri_load(a.kf_Tcw + 7 * (size_t)(it.kf0 + kf)), w);
                                d = tri_pdist(a.obs_px[oB + j], kp_project_dist(a.cal, cc.x, cc.y, cc.z));
                            }
                        }
                        unsigned long long m = __ballot(valid);
                        while (m) {                                                  // ascending keyframe id: the order of the sum
                            const int s = __ffsll((long long)m) - 1;
                            m &= m - 1;
                            coprojpx = (float)((double)coprojpx + __shfl(d, s));
                            nbcokp++;
                        }
                    }
                    if (coprojpx / (float)nbcokp > it.dmax) continue;                // 0 / 0: NaN, passes
                }
                int hm = 1000;                                                       // MapPoint::computeMinDescDist
                const long long npairs = (long long)nDA * nDB;
                const int dB = it.de0 + a.desc_start[B];
                for (long long p = lane; p < npairs; p += 64) {
                    const int i = (int)(p / nDB), j = (int)(p - (long long)i * nDB);
                    const uint4 a0 = a.desc[2 * (size_t)(dA + i)], a1 = a.desc[2 * (size_t)(dA + i) + 1];
                    const uint4 b0 = a.desc[2 * (size_t)(dB + j)], b1 = a.desc[2 * (size_t)(dB + j) + 1];
                    const int h = __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
                                  __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
                    hm = h < hm ? h : hm;
                }
                for (int o = 32; o > 0; o >>= 1) {
                    const int v = __shfl_xor(hm, o);
                    hm = v < hm ? v : hm;
                }
                const float dist = (float)hm;
                if (dist <= bestdist) {                                              // :722-732 / :711-721
                    secdist = bestdist; secid = bestid;
                    bestdist = dist; bestid = k;
                } else if (dist <= secdist) {
                    secdist = dist; secid = k;
                }
            }
        }
        if (bestid == -1) st = OV2_MATCH_NO_CANDIDATE;
        else if (secid != -1 && 0.9 * (double)secdist < (double)bestdist) st = OV2_MATCH_RATIO_REJECTED;   // :735-739 / :724-728
        else st = OV2_MATCH_BEST;
    }
    if (lane == 0) {
        a.lm_status[gl] = (uint8_t)st;
        a.lm_kp[gl] = (st & OV2_MATCH_BEST) ? bestid : -1;
        a.lm_dist[gl] = bestdist;
        a.lm_projpx[gl] = ppx;
        if (st & OV2_MATCH_BEST)
            atomicMin(a.keys + it.kp0 + bestid, ((unsigned long long)(unsigned)(int)bestdist << 32) | (0xFFFFFFFFull - (unsigned)l));
    }
}

// keys[i] = ~0 (nobody proposed keypoint i) or (distance << 32) | (0xFFFFFFFF - local-map index)
__global__ __launch_bounds__(256) void k_map_pick(const unsigned long long *__restrict__ keys, int n, int *__restrict__ kp_lm,
                                                  float *__restrict__ kp_dist)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = keys[i];
    const bool none = key == ~0ull;
    kp_lm[i] = none ? -1 : (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
    kp_dist[i] = none ? 0.f : (float)(unsigned)(key >> 32);
}

// offsets[0 .. n]: starts at 0, never decreases
static bool mt_offsets_ok(const int *o, int n)
{
    if (o[0] != 0) return false;
    for (int i = 0; i < n; i++)
        if (o[i + 1] < o[i]) return false;
    return true;
}

// the pose table exists on the mapper's side only
static inline int mt_n_kf(const ov2_match_keyframe &k) { return k.n_kf; }
static inline int mt_n_kf(const ov2_loopmap_item &) { return 0; }

// Both call families.  Item is ov2_match_keyframe (the mapper) or ov2_loopmap_item (the loop closer); the params and result types
// of a family hold the same fields under the same names.
template <class Params, class Item, class Result>
static int mt_run(ov2_ctx *ctx, const Params *params, int n_items, const Item *items, Result *results)
{
    constexpr bool LOOP = std::is_same<Item, ov2_loopmap_item>::value;
    // the inputs first, the context last: a malformed input is reported without a device
    OV2_REQUIRE(params, OV2_EINVAL, "NULL params");
    OV2_REQUIRE(n_items >= 0, OV2_EINVAL, "n_items < 0");
    OV2_REQUIRE(n_items == 0 || (items && results), OV2_EINVAL, "NULL item / result array");
    OV2_REQUIRE(n_items <= 65535, OV2_EUNSUPPORTED, "more than 65535 items in one call");
    OV2_REQUIRE(params->desc_bytes == 32, OV2_EUNSUPPORTED, "descriptors of 32 bytes only");
    OV2_REQUIRE(params->model == OV2_CAM_PINHOLE || params->model == OV2_CAM_FISHEYE, OV2_EINVAL, "unknown camera model");
    OV2_REQUIRE(params->nD >= 0 && (params->nD == 0 || params->D), OV2_EINVAL, "bad distortion vector");
    {
        const int nD = params->nD;
        const bool ok = nD == 0 || (params->model == OV2_CAM_FISHEYE ? nD == 4 : (nD == 4 || nD == 5 || nD == 8 || nD == 12));
        OV2_REQUIRE(ok, OV2_EUNSUPPORTED, "unsupported coefficient count: pinhole takes 0 / 4 / 5 / 8 / 12 distortion coefficients, fisheye 0 / 4");
    }
    OV2_REQUIRE(params->img_w > 0 && params->img_h > 0 && params->ncellsize > 0, OV2_EINVAL, "img_w / img_h / ncellsize not positive");
    OV2_REQUIRE(params->img_w <= 65536 && params->img_h <= 65536, OV2_EINVAL, "img_w / img_h above 65536");
    // Frame's grid (frame.cpp:41-43)
    const int nbw = (int)ceilf((float)params->img_w / (float)params->ncellsize);
    const int nbh = (int)ceilf((float)params->img_h / (float)params->ncellsize);
    OV2_REQUIRE((double)nbw * params->ncellsize >= params->img_w && (double)nbh * params->ncellsize >= params->img_h, OV2_EINVAL,
                "img_w / img_h: the float grid of the Frame does not cover the image");
    const size_t ncells = (size_t)nbw * (size_t)nbh;
    size_t NKP = 0, NCK = 0, NMP = 0, NOB = 0, NDE = 0, NKF = 0, NLM = 0;
    int lm_max = 0;
    for (int b = 0; b < n_items; b++) {
        const Item &k = items[b];
        const Result &r = results[b];
        const int n_kf = mt_n_kf(k);
        OV2_REQUIRE(k.Tcw, OV2_EINVAL, "Tcw == NULL");
        OV2_REQUIRE(k.n_kp >= 0 && k.n_mp >= 0 && n_kf >= 0 && k.n_lm >= 0, OV2_EINVAL, "negative count (n_kp / n_mp / n_kf / n_lm)");
        int n_ck = 0, n_ob = 0, n_de = 0;
        if (k.n_kp > 0) {
            bool have = k.kp_px && k.kp_mp && k.cell_start;
            if constexpr (LOOP) have = have && k.kp_matched;
            OV2_REQUIRE(have, OV2_EINVAL, "NULL kp_px / kp_mp / kp_matched / cell_start");
            OV2_REQUIRE(r.kp_lm && r.kp_dist, OV2_EINVAL, "NULL result buffer (kp_lm / kp_dist)");
        }
        if (k.cell_start) {
            OV2_REQUIRE(mt_offsets_ok(k.cell_start, (int)ncells), OV2_EINVAL, "cell_start does not start at 0 or decreases");
            n_ck = k.cell_start[ncells];
            OV2_REQUIRE(n_ck == 0 || k.cell_kp, OV2_EINVAL, "cell_kp == NULL");
            for (int i = 0; i < n_ck; i++)
                OV2_REQUIRE(k.cell_kp[i] >= 0 && k.cell_kp[i] < k.n_kp, OV2_EINVAL, "cell_kp: keypoint row outside the keypoint table");
        }
        if (k.n_mp > 0) {
            OV2_REQUIRE(k.obs_start && k.desc_start, OV2_EINVAL, "NULL obs_start / desc_start");
            OV2_REQUIRE(mt_offsets_ok(k.obs_start, k.n_mp), OV2_EINVAL, "obs_start does not start at 0 or decreases");
            OV2_REQUIRE(mt_offsets_ok(k.desc_start, k.n_mp), OV2_EINVAL, "desc_start does not start at 0 or decreases");
            n_ob = k.obs_start[k.n_mp]; n_de = k.desc_start[k.n_mp];
            bool have = k.obs_kfid;
            if constexpr (!LOOP) have = have && k.obs_kf && k.obs_px;
            OV2_REQUIRE(n_ob == 0 || have, OV2_EINVAL, "NULL obs_kfid / obs_kf / obs_px");
            OV2_REQUIRE(n_de == 0 || k.desc, OV2_EINVAL, "desc == NULL");
            for (int m = 0; m < k.n_mp; m++)
                for (int j = k.obs_start[m]; j < k.obs_start[m + 1]; j++) {
                    if constexpr (!LOOP)
                        OV2_REQUIRE(k.obs_kf[j] >= -1 && k.obs_kf[j] < n_kf, OV2_EINVAL, "obs_kf: row outside the pose table");
                    OV2_REQUIRE(j == k.obs_start[m] || k.obs_kfid[j - 1] < k.obs_kfid[j], OV2_EINVAL, "obs_kfid unsorted: not strictly ascending inside a row");
                }
        }
        if constexpr (!LOOP) OV2_REQUIRE(n_kf == 0 || k.kf_Tcw, OV2_EINVAL, "kf_Tcw == NULL");
        for (int i = 0; i < k.n_kp; i++)
            OV2_REQUIRE(k.kp_mp[i] >= -1 && k.kp_mp[i] < k.n_mp, OV2_EINVAL, "kp_mp: row outside the map-point table");
        if (k.n_lm > 0) {
            OV2_REQUIRE(k.lm_mp && k.lm_wpt, OV2_EINVAL, "NULL lm_mp / lm_wpt");
            OV2_REQUIRE(r.lm_status && r.lm_kp && r.lm_dist && r.lm_projpx, OV2_EINVAL, "NULL result buffer (lm_status / lm_kp / lm_dist / lm_projpx)");
            for (int i = 0; i < k.n_lm; i++)
                OV2_REQUIRE(k.lm_mp[i] >= 0 && k.lm_mp[i] < k.n_mp, OV2_EINVAL, "lm_mp: row outside the map-point table");
        }
        NKP += (size_t)k.n_kp; NCK += (size_t)n_ck; NMP += (size_t)k.n_mp; NOB += (size_t)n_ob; NDE += (size_t)n_de;
        NKF += (size_t)n_kf; NLM += (size_t)k.n_lm;
        lm_max = k.n_lm > lm_max ? k.n_lm : lm_max;
    }
    const size_t B = (size_t)n_items, lim = 0x7fffffff;
    OV2_REQUIRE(NKP <= lim && NCK <= lim && NMP + B <= lim && NOB <= lim && NDE <= lim && NKF <= lim && NLM <= lim && B * (ncells + 1) <= lim,
                OV2_EUNSUPPORTED, "more than 2^31 - 1 elements of one kind in one call");
    OV2_REQUIRE(ctx, OV2_EINVAL, "NULL context");
    if (n_items == 0) return OV2_OK;

    MapMatchArgs a = {};
    {
        const double iK[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};             // the inverse model's matrix: not read here
        const int rc = ov2_kp_calib(params->model, params->K, params->D, params->nD, iK, a.cal);
        if (rc) return rc;
    }
    // The two cones differ on purpose.  loop_closer.cpp:595-607 and :656, in float as written: the field of view MULTIPLIED by the
    // focal length, atan(hfov) in both branches
    if constexpr (LOOP) {
        const float hfov = (float)(0.5 * params->img_w * params->K[0]);
        const float maxradfov = (float)std::atan((double)hfov);
        a.view_th = (float)std::cos((double)maxradfov);
    } else {                // mapper.cpp:586-602, in float as written
        const float vfov = (float)(0.5 * params->img_h / params->K[1]), hfov = (float)(0.5 * params->img_w / params->K[0]);
        const float maxradfov = hfov > vfov ? std::atan(hfov) : std::atan(vfov);
        a.view_th = std::cos(maxradfov);
    }
    a.mindist = (float)((double)((float)params->desc_bytes * params->fmax_desc_dist) * 8.);
    a.img_w = params->img_w; a.img_h = params->img_h; a.cellsize = (float)params->ncellsize; a.nbw = nbw;

    // staging: [items 96 B][kp_px 8][kp_mp 4][kp_matched 1, loop closer][cell_start 4][cell_kp 4][obs_start 4][desc_start 4][obs_kfid 4]
    // [obs_kf 4, mapper][obs_px 8, mapper][desc 32][kf_Tcw 56, mapper][lm_mp 4][lm_wpt 24][keys 8, all ones], then the outputs
    // [lm_status 1][lm_kp 4][lm_dist 4][lm_projpx 8][kp_lm 4][kp_dist 4]; every section 16-byte aligned, a section of the other mode empty
    const size_t CS = B * (ncells + 1), MS = NMP + B, NKM = LOOP ? NKP : 0, NOM = LOOP ? 0 : NOB;
    StageCursor c(16);
    const size_t o_it = c.take(sizeof(MapMatchItem) * B), o_kpx = c.take(8 * NKP), o_kmp = c.take(4 * NKP), o_kma = c.take(NKM);
    const size_t o_cs = c.take(4 * CS), o_ck = c.take(4 * NCK), o_os = c.take(4 * MS), o_ds = c.take(4 * MS), o_oid = c.take(4 * NOB);
    const size_t o_okf = c.take(4 * NOM), o_opx = c.take(8 * NOM), o_de = c.take(32 * NDE), o_kf = c.take(56 * NKF), o_lmp = c.take(4 * NLM);
    const size_t o_lw = c.take(24 * NLM), o_key = c.take(8 * NKP);
    const size_t o_out = c.take(NLM), o_lk = c.take(4 * NLM), o_ld = c.take(4 * NLM), o_lp = c.take(8 * NLM), o_kl = c.take(4 * NKP);
    const size_t o_kd = c.take(4 * NKP), total = c.off;
    Stage st;
    int rc = st.open(ctx, total, total);  if (rc) return rc;
    uint8_t *hs = st.h, *ds = st.d;
    size_t kp0 = 0, ck0 = 0, mp0 = 0, ob0 = 0, de0 = 0, kf0 = 0, lm0 = 0;
    for (int b = 0; b < n_items; b++) {
        const Item &k = items[b];
        const size_t n_ck = k.cell_start ? (size_t)k.cell_start[ncells] : 0, n_kf = (size_t)mt_n_kf(k);
        const size_t n_ob = k.n_mp ? (size_t)k.obs_start[k.n_mp] : 0, n_de = k.n_mp ? (size_t)k.desc_start[k.n_mp] : 0;
        MapMatchItem it;
        memset(&it, 0, sizeof(it));
        memcpy(it.Tcw, k.Tcw, 56);
        it.dmax = params->fmax_proj_pxdist;
        if constexpr (!LOOP)
            if (k.nb3dkps < 30) it.dmax = (float)((double)it.dmax * 2.);   // mapper.cpp:599-602
        it.n_lm = k.n_lm;
        it.kp0 = (int)kp0; it.cell0 = (int)((size_t)b * (ncells + 1)); it.ck0 = (int)ck0; it.mp0 = (int)(mp0 + (size_t)b);
        it.ob0 = (int)ob0; it.de0 = (int)de0; it.kf0 = (int)kf0; it.lm0 = (int)lm0;
        memcpy(hs + o_it + sizeof(MapMatchItem) * b, &it, sizeof(MapMatchItem));
        if (k.n_kp) {
            memcpy(hs + o_kpx + 8 * kp0, k.kp_px, 8 * (size_t)k.n_kp);
            memcpy(hs + o_kmp + 4 * kp0, k.kp_mp, 4 * (size_t)k.n_kp);
            if constexpr (LOOP) memcpy(hs + o_kma + kp0, k.kp_matched, (size_t)k.n_kp);
        }
        if (k.cell_start) memcpy(hs + o_cs + 4 * (size_t)it.cell0, k.cell_start, 4 * (ncells + 1));
        else memset(hs + o_cs + 4 * (size_t)it.cell0, 0, 4 * (ncells + 1));
        if (n_ck) memcpy(hs + o_ck + 4 * ck0, k.cell_kp, 4 * n_ck);
        if (k.n_mp) {
            memcpy(hs + o_os + 4 * (size_t)it.mp0, k.obs_start, 4 * ((size_t)k.n_mp + 1));
            memcpy(hs + o_ds + 4 * (size_t)it.mp0, k.desc_start, 4 * ((size_t)k.n_mp + 1));
        } else {
            memset(hs + o_os + 4 * (size_t)it.mp0, 0, 4);
            memset(hs + o_ds + 4 * (size_t)it.mp0, 0, 4);
        }
        if (n_ob) memcpy(hs + o_oid + 4 * ob0, k.obs_kfid, 4 * n_ob);
        if (n_de) memcpy(hs + o_de + 32 * de0, k.desc, 32 * n_de);
        if constexpr (!LOOP) {
            if (n_ob) {
                memcpy(hs + o_okf + 4 * ob0, k.obs_kf, 4 * n_ob);
                memcpy(hs + o_opx + 8 * ob0, k.obs_px, 8 * n_ob);
            }
            if (n_kf) memcpy(hs + o_kf + 56 * kf0, k.kf_Tcw, 56 * n_kf);
        }
        if (k.n_lm) {
            memcpy(hs + o_lmp + 4 * lm0, k.lm_mp, 4 * (size_t)k.n_lm);
            memcpy(hs + o_lw + 24 * lm0, k.lm_wpt, 24 * (size_t)k.n_lm);
        }
        kp0 += (size_t)k.n_kp; ck0 += n_ck; mp0 += (size_t)k.n_mp; ob0 += n_ob; de0 += n_de; kf0 += n_kf; lm0 += (size_t)k.n_lm;
    }
    memset(hs + o_key, 0xff, 8 * NKP);
    rc = st.upload(0, o_out);  if (rc) return rc;
    if (NKP + NLM > 0) {
        a.items = (const MapMatchItem *)(ds + o_it);
        a.kp_px = (const float2 *)(ds + o_kpx); a.kp_mp = (const int *)(ds + o_kmp);
        a.cell_start = (const int *)(ds + o_cs); a.cell_kp = (const int *)(ds + o_ck);
        a.obs_start = (const int *)(ds + o_os); a.desc_start = (const int *)(ds + o_ds);
        a.obs_kfid = (const int *)(ds + o_oid); a.desc = (const uint4 *)(ds + o_de);
        if constexpr (LOOP) {
            a.kp_matched = ds + o_kma;
        } else {
            a.obs_kf = (const int *)(ds + o_okf); a.obs_px = (const float2 *)(ds + o_opx); a.kf_Tcw = (const double *)(ds + o_kf);
        }
        a.lm_mp = (const int *)(ds + o_lmp); a.lm_wpt = (const double *)(ds + o_lw);
        a.keys = (unsigned long long *)(ds + o_key);
        a.lm_status = ds + o_out; a.lm_kp = (int *)(ds + o_lk); a.lm_dist = (float *)(ds + o_ld); a.lm_projpx = (float2 *)(ds + o_lp);
        if (lm_max > 0) {
            hipLaunchKernelGGL(k_map_match<LOOP>, dim3((lm_max + MT_WAVES - 1) / MT_WAVES, n_items), dim3(MT_BLOCK), 0, ctx->stream, a);
            OV2_HIP_CHECK(hipGetLastError());
        }
        if (NKP > 0) {
            hipLaunchKernelGGL(k_map_pick, dim3((unsigned)((NKP + 255) / 256)), dim3(256), 0, ctx->stream, a.keys, (int)NKP,
                               (int *)(ds + o_kl), (float *)(ds + o_kd));
            OV2_HIP_CHECK(hipGetLastError());
        }
        rc = st.download(o_out, total, o_out);  if (rc) return rc;
    }
    rc = st.sync();  if (rc) return rc;
    kp0 = lm0 = 0;
    for (int b = 0; b < n_items; b++) {
        const size_t nk = (size_t)items[b].n_kp, nl = (size_t)items[b].n_lm;
        Result &r = results[b];
        r.n_matches = 0;
        if (nl) {
            memcpy(r.lm_status, hs + o_out + lm0, nl);
            memcpy(r.lm_kp, hs + o_lk + 4 * lm0, 4 * nl);
            memcpy(r.lm_dist, hs + o_ld + 4 * lm0, 4 * nl);
            memcpy(r.lm_projpx, hs + o_lp + 8 * lm0, 8 * nl);
        }
        if (nk) {
            memcpy(r.kp_lm, hs + o_kl + 4 * kp0, 4 * nk);
            memcpy(r.kp_dist, hs + o_kd + 4 * kp0, 4 * nk);
            for (size_t i = 0; i < nk; i++) r.n_matches += r.kp_lm[i] >= 0 ? 1 : 0;
        }
        kp0 += nk; lm0 += nl;
    }
    return OV2_OK;
}

int ov2_match_to_map_batch(ov2_ctx *ctx, const ov2_match_params *params, int n_items, const ov2_match_keyframe *kfs,
                           ov2_match_result *results)
{
    return mt_run(ctx, params, n_items, kfs, results);
}

int ov2_match_to_map(ov2_ctx *ctx, const ov2_match_params *params, const ov2_match_keyframe *kf, ov2_match_result *result)
{
    OV2_REQUIRE(kf && result, OV2_EINVAL, "NULL keyframe / result");
    return mt_run(ctx, params, 1, kf, result);
}

int ov2_loop_match_to_map_batch(ov2_ctx *ctx, const ov2_loopmap_params *params, int n_items, const ov2_loopmap_item *items,
                                ov2_loopmap_result *results)
{
    return mt_run(ctx, params, n_items, items, results);
}

int ov2_loop_match_to_map(ov2_ctx *ctx, const ov2_loopmap_params *params, const ov2_loopmap_item *item, ov2_loopmap_result *result)
{
    OV2_REQUIRE(item && result, OV2_EINVAL, "NULL item / result");
    return mt_run(ctx, params, 1, item, result);
}
