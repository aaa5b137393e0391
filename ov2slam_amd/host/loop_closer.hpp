// loop_closer.hpp -- C++ adapter for the loop closer's descriptor matching (LoopCloser::knnMatching, src/loop_closer.cpp:378-459)
// over ov2_knn_match[_batch].  The reference walks the two frames inside the function (:391-420): which keypoints of the new
// keyframe the candidate already observes, and which map points carry a descriptor.  Here the caller does those two walks and
// hands over what they collect: the query rows with their vkpids, the train rows with their vlmids.  The call appends
// (vkpids[q], vlmids[t]) of the good rows to vkplmids in query order, exactly what :444-448 appends.
//
// And for the keyframe preparation in front of it (LoopCloser::run, src/loop_closer.cpp:86-144) over ov2_lckf_prepare /
// ov2_tracker_lckf_prepare: detectAdditionalKeypoints takes the raw image (or the tracker that holds it on the device) and the
// pixels of the keypoints whose map point already has a descriptor -- the frame walk :96-113 stays with the caller -- and returns
// what the reference calls vaddkps / adddescs: the extra FAST corners that survive the mask, retainBest(300) and BRIEF's border
// filter, with their descriptors.  The library's lists are in raster order; Order::Reference reorders them on the host with the
// literal std::nth_element / std::partition of KeyPointsFilter::retainBest (retainBestReferenceOrder below), which gives the
// reference's keypoint order when both are built with the same libstdc++.
//
// And for the local-map tracking behind P3P (LoopCloser::trackLoopLocalMap / matchToMap, src/loop_closer.cpp:502-763) over
// ov2_loop_match_to_map[_batch]: the caller flattens the new keyframe's keypoints and the local map (LoopMapInput), the call appends
// (keypoint's lmid, local map point's lmid) of the matches to vkplmids in ascending keypoint id, exactly what :576-582 appends.  The
// covisible-keyframe walk in front of it (:505-562) needs no device: loopLocalMapReferenceOrder below does it with literal
// std::unordered_set inserts and erases, so the local map comes out in the iteration order the reference walks it in when both are
// built with the same libstdc++ -- the order that decides which of two equally distant points keeps a keypoint.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <map>
#include <unordered_set>
#include "ov2_types.hpp"

namespace ov2 {

// one query / train pair of the batch form: descriptor rows of 32 bytes, one id per row
struct KnnMatchingInput {
    std::vector<uint8_t> query; std::vector<int> vkpids;
    std::vector<uint8_t> train; std::vector<int> vlmids;
};

// one FAST corner as the library lists it
struct LckfCorner { int16_t x, y; uint8_t response; };

// KeyPointsFilter::retainBest(keypoints, n_points) of OpenCV's keypoint.cpp, literally, on the corners in the order cv::FAST and
// runByPixelsMask leave them (raster): the same comparisons in the same order as the reference makes, so the same permutation.
// Needs no device.
inline void retainBestReferenceOrder(std::vector<LckfCorner> &keypoints, int n_points)
{
    if (n_points >= 0 && keypoints.size() > (size_t)n_points) {
        if (n_points == 0) { keypoints.clear(); return; }
        std::nth_element(keypoints.begin(), keypoints.begin() + n_points - 1, keypoints.end(),
                         [](const LckfCorner &a, const LckfCorner &b) { return a.response > b.response; });     // KeypointResponseGreater
        const uint8_t ambiguous_response = keypoints[(size_t)n_points - 1].response;
        const auto new_end = std::partition(keypoints.begin() + n_points, keypoints.end(),
                                            [ambiguous_response](const LckfCorner &k) { return k.response >= ambiguous_response; });
        keypoints.resize((size_t)(new_end - keypoints.begin()));
    }
}

// LoopCloser::matchToMap: the arrays of ov2_loopmap_item (include/ov2slam_hip.h) plus the ids the rows stand for
struct LoopMapInput {
    double Tcw[7] = {0, 0, 0, 0, 0, 0, 1};  // Twc.inverse() of the P3P / PnP result
    std::vector<int> kp_lmid;           // n_kp: the keypoints' lmid_ (the keys of map_previd_newid)
    std::vector<Point2f> kp_px;         // n_kp
    std::vector<int> kp_mp;             // n_kp: row of the map-point table, -1 = no usable map point
    std::vector<uint8_t> kp_matched;    // n_kp: non-zero = the keypoint's lmid_ is in vmatchedkpids
    std::vector<int> cell_start, cell_kp;   // ncells + 1 offsets; keypoint rows per cell in vgridkps_ order
    std::vector<int> obs_start;         // n_mp + 1
    std::vector<int> obs_kfid;          // per observation: keyframe id, ascending inside a row
    std::vector<int> desc_start;        // n_mp + 1
    std::vector<uint8_t> desc;          // 32 per descriptor
    std::vector<int> lm_lmid;           // n_lm: the local map points' ids, in iteration order (the values of map_previd_newid)
    std::vector<int> lm_mp;             // n_lm: row of the map-point table
    std::vector<double> lm_wpt;         // 3 n_lm
};

struct LoopMapOutput {
    std::vector<uint8_t> lm_status;     // n_lm: OV2_LOOPMAP_* bits
    std::vector<int> lm_kp;             // n_lm: proposed keypoint row or -1
    std::vector<float> lm_dist, lm_projpx;   // n_lm, 2 n_lm
    std::vector<int> kp_lm;             // n_kp: winning local-map index or -1
    std::vector<float> kp_dist;         // n_kp
    std::map<int, int> map_previd_newid;    // keypoint's lmid -> local map point's lmid
};

// one entry of lckf.getCovisibleKfMap() as the walk meets it: the keyframe id and the lmid_ of its getKeypoints3d(), in order;
// kp3d_lmids == nullptr stands for pmap_->getKeyframe(kfid) == nullptr
struct LoopCovisibleKeyframe { int kfid; const std::vector<int> *kp3d_lmids; };

// The set-building walk of LoopCloser::trackLoopLocalMap (:505-562), literally: lccov in ascending keyframe id (std::map order;
// the loop keyframe's own entry included, which the reference adds at :509), newkf_observes = newkf.isObservingKp.  Appends the
// (lmid, lmid) pairs to vkplmids, fills vmatchedkpids (if given) and returns set_local_lmids in its iteration order.  Needs no device.
inline std::vector<int> loopLocalMapReferenceOrder(int lckf_kfid, const std::vector<LoopCovisibleKeyframe> &lccov,
                                                   const std::function<bool(int)> &newkf_observes,
                                                   std::vector<std::pair<int, int>> &vkplmids, std::vector<int> *vmatchedkpids = nullptr)
{
    std::unordered_set<int> set_local_lmids, set_checked_kpids;
    for (const LoopCovisibleKeyframe &cokf : lccov) {
        const int kfid = cokf.kfid;
        if (kfid < lckf_kfid - 15) {
            continue;
        } else if (kfid > lckf_kfid + 15) {
            break;
        }
        if (cokf.kp3d_lmids == nullptr) {
            continue;
        }
        for (const int lmid : *cokf.kp3d_lmids) {
            auto it = set_checked_kpids.find(lmid);
            if (it == set_checked_kpids.end()) {
                set_checked_kpids.insert(lmid);
                if (newkf_observes(lmid)) {
                    std::pair<int, int> kplmid(lmid, lmid);
                    auto kpit = std::find(vkplmids.begin(), vkplmids.end(), kplmid);
                    if (kpit == vkplmids.end()) {
                        vkplmids.push_back(kplmid);
                    }
                } else {
                    set_local_lmids.insert(lmid);
                }
            }
        }
    }
    if (vmatchedkpids) {
        vmatchedkpids->clear();
        vmatchedkpids->reserve(vkplmids.size());
    }
    for (const auto &kplmid : vkplmids) {
        if (vmatchedkpids) vmatchedkpids->push_back(kplmid.first);
        set_local_lmids.erase(kplmid.second);
    }
    std::vector<int> order;
    order.reserve(set_local_lmids.size());
    for (const int lmid : set_local_lmids) order.push_back(lmid);
    return order;
}

class LoopCloser {
public:
    enum class Order { Raster, Reference };

    // the reference's settings: 32-byte BRIEF rows, maxdist = query.cols * 0.5 * 8., ratio 0.85
    explicit LoopCloser(int desc_bytes = 32, double ratio = 0.85)
    {
        kp_.desc_bytes = desc_bytes; kp_.max_dist = (int)(desc_bytes * 0.5 * 8.); kp_.ratio = ratio;
    }

    // the matcher, the distance gate and the ratio test of one loop candidate (one upload, one synchronisation); OV2_OK or the
    // library's error, in which case vkplmids is left as it was.  Empty query or train rows: nothing is appended (:422-424).
    int knnMatching(Context &ctx, const std::vector<uint8_t> &query, const std::vector<int> &vkpids, const std::vector<uint8_t> &train,
                    const std::vector<int> &vlmids, std::vector<std::pair<int, int>> &vkplmids) const
    {
        const View v{&query, &vkpids, &train, &vlmids};
        std::vector<std::pair<int, int>> *out = &vkplmids;
        return run(ctx, &v, 1, &out);
    }
    // several candidates in one call, e.g. one keyframe against many, or the candidates of a lock-step batch: vkplmids[b] is
    // appended to as the single form does for item b (the vector is grown to in.size() entries)
    int knnMatching(Context &ctx, const std::vector<KnnMatchingInput> &in, std::vector<std::vector<std::pair<int, int>>> &vkplmids) const
    {
        if (vkplmids.size() < in.size()) vkplmids.resize(in.size());
        std::vector<View> v(in.size());
        std::vector<std::vector<std::pair<int, int>> *> out(in.size());
        for (size_t b = 0; b < in.size(); b++) {
            v[b] = View{&in[b].query, &in[b].vkpids, &in[b].train, &in[b].vlmids};
            out[b] = &vkplmids[b];
        }
        return run(ctx, v.data(), in.size(), out.data());
    }

    // The extra keypoints of a new keyframe and their descriptors (:115-131): FAST(20) under the mask of excl_px, retainBest(300),
    // BRIEF.  Only the keypoints BRIEF describes come back (compute() drops the others): out_px their pixels, out_resp their FAST
    // responses, out_desc 32 bytes each.  OV2_OK or the library's error, in which case the outputs are left as they were.
    int detectAdditionalKeypoints(Context &ctx, const Image8 &img, const std::vector<Point2f> &excl_px, std::vector<Point2f> &out_px,
                                  std::vector<float> &out_resp, std::vector<uint8_t> &out_desc, Order order = Order::Raster) const
    {
        if (img.empty()) return OV2_EINVAL;
        return lckf(order, out_px, out_resp, out_desc, [&](ov2_lckf_result *r) {
            return ov2_lckf_prepare(ctx.get(), img.data, img.cols, img.rows, img.step, &lp_, excl_px.empty() ? nullptr : &excl_px[0].x,
                                    (int)excl_px.size(), r);
        });
    }
    // the same on the raw frame the tracker already holds on the device (no image upload)
    int detectAdditionalKeypoints(ov2_tracker *trk, const std::vector<Point2f> &excl_px, std::vector<Point2f> &out_px,
                                  std::vector<float> &out_resp, std::vector<uint8_t> &out_desc, Order order = Order::Raster) const
    {
        return lckf(order, out_px, out_resp, out_desc, [&](ov2_lckf_result *r) {
            return ov2_tracker_lckf_prepare(trk, &lp_, excl_px.empty() ? nullptr : &excl_px[0].x, (int)excl_px.size(), r);
        });
    }
    // the settings of FastFeatureDetector::create(20), retainBest(vaddkps, 300) and cv::circle(mask, px, 2., 0, -1)
    void setKeyframePreparation(int threshold, int retain, int excl_radius) { lp_.threshold = threshold; lp_.retain = retain; lp_.excl_radius = excl_radius; }

    // what trackLoopLocalMap needs: the left camera's model (OV2_CAM_*) / K / distortion vector / image size, Frame::ncellsize_, and
    // maxdist / ratio as processLoopCandidate passes them (10. and (float)(fmax_desc_dist_ * 1.5), fmax_desc_dist_ = 0.2 by default)
    void setLoopMapMatching(int model, const double K[4], const double *D, int nD, double img_w, double img_h, int ncellsize,
                            float fmaxprojerr = 10.f, float fdistratio = (float)(0.2 * 1.5))
    {
        std::memset(&mp_, 0, sizeof(mp_));
        mp_.model = model; std::memcpy(mp_.K, K, sizeof(mp_.K));
        md_.assign(D, D + (nD > 0 ? nD : 0));
        mp_.nD = nD; mp_.img_w = img_w; mp_.img_h = img_h; mp_.ncellsize = ncellsize;
        mp_.fmax_proj_pxdist = fmaxprojerr; mp_.fmax_desc_dist = fdistratio; mp_.desc_bytes = 32;
        has_loopmap_ = true;
    }
    // LoopCloser::matchToMap of one loop candidate and the append :576-582 (one upload, one synchronisation): (kp_lmid, lm_lmid) of
    // the matches go to the end of vkplmids in ascending keypoint id.  OV2_OK or the library's error (OV2_EINVAL before
    // setLoopMapMatching), in which case vkplmids and *out are left as they were.
    int trackLoopLocalMap(Context &ctx, const LoopMapInput &in, std::vector<std::pair<int, int>> &vkplmids, LoopMapOutput *out = nullptr) const
    {
        std::vector<LoopMapOutput> o(1);
        const int rc = runLoopMap(ctx, &in, 1, o.data());
        if (rc != OV2_OK) return rc;
        for (const auto &e : o[0].map_previd_newid) vkplmids.emplace_back(e.first, e.second);
        if (out) *out = std::move(o[0]);
        return OV2_OK;
    }
    // several candidates in one call: vkplmids[b] is appended to as the single form does for item b (the vector is grown to
    // in.size() entries)
    int trackLoopLocalMap(Context &ctx, const std::vector<LoopMapInput> &in, std::vector<std::vector<std::pair<int, int>>> &vkplmids,
                          std::vector<LoopMapOutput> *out = nullptr) const
    {
        std::vector<LoopMapOutput> o(in.size());
        const int rc = runLoopMap(ctx, in.data(), in.size(), o.data());
        if (rc != OV2_OK) return rc;
        if (vkplmids.size() < in.size()) vkplmids.resize(in.size());
        for (size_t b = 0; b < in.size(); b++)
            for (const auto &e : o[b].map_previd_newid) vkplmids[b].emplace_back(e.first, e.second);
        if (out) *out = std::move(o);
        return OV2_OK;
    }

private:
    ov2_knn_params kp_ = {};
    ov2_lckf_params lp_ = {20, 300, 2};
    ov2_loopmap_params mp_ = {};
    std::vector<double> md_;
    bool has_loopmap_ = false;

    static const float *fp(const std::vector<Point2f> &v) { return v.empty() ? nullptr : &v[0].x; }
    template <class T> static const T *dp(const std::vector<T> &v) { return v.empty() ? nullptr : v.data(); }

    static bool loopmap_sizes_ok(const LoopMapInput &k)
    {
        const size_t n_kp = k.kp_lmid.size(), n_lm = k.lm_lmid.size();
        if (k.kp_px.size() != n_kp || k.kp_mp.size() != n_kp || k.kp_matched.size() != n_kp) return false;
        if (k.lm_mp.size() != n_lm || k.lm_wpt.size() != 3 * n_lm || k.obs_start.size() != k.desc_start.size()) return false;
        if (!k.obs_start.empty() && (k.obs_start.back() < 0 || k.desc_start.back() < 0)) return false;
        const size_t n_ob = k.obs_start.empty() ? 0 : (size_t)k.obs_start.back(), n_de = k.desc_start.empty() ? 0 : (size_t)k.desc_start.back();
        if (k.obs_kfid.size() != n_ob || k.desc.size() != 32 * n_de) return false;
        if (!k.cell_start.empty() && (k.cell_start.back() < 0 || k.cell_kp.size() != (size_t)k.cell_start.back())) return false;
        return n_kp <= 0x7fffffff && n_lm <= 0x7fffffff && k.obs_start.size() <= 0x7fffffff;
    }

    int runLoopMap(Context &ctx, const LoopMapInput *in, size_t n_items, LoopMapOutput *out) const
    {
        static_assert(sizeof(Point2f) == 2 * sizeof(float), "Point2f must be two packed floats");
        if (!has_loopmap_ || n_items > 0x7fffffff) return OV2_EINVAL;
        ov2_loopmap_params mp = mp_;
        mp.D = md_.empty() ? nullptr : md_.data();
        std::vector<ov2_loopmap_item> items(n_items);
        std::vector<ov2_loopmap_result> res(n_items);
        for (size_t b = 0; b < n_items; b++) {
            const LoopMapInput &k = in[b];
            if (!loopmap_sizes_ok(k)) return OV2_EINVAL;
            // the library reads ncells + 1 offsets: a cell table of another length is the caller's error, not a read past the end
            const size_t nbw = (size_t)std::ceil((float)mp.img_w / (float)mp.ncellsize), nbh = (size_t)std::ceil((float)mp.img_h / (float)mp.ncellsize);
            if (!k.cell_start.empty() && k.cell_start.size() != nbw * nbh + 1) return OV2_EINVAL;
            if (k.cell_start.empty() && !k.kp_lmid.empty()) return OV2_EINVAL;
            ov2_loopmap_item &s = items[b];
            s.Tcw = k.Tcw;
            s.n_kp = (int)k.kp_lmid.size(); s.kp_px = fp(k.kp_px); s.kp_mp = dp(k.kp_mp); s.kp_matched = dp(k.kp_matched);
            s.cell_start = dp(k.cell_start); s.cell_kp = dp(k.cell_kp);
            s.n_mp = k.obs_start.empty() ? 0 : (int)k.obs_start.size() - 1;
            s.obs_start = dp(k.obs_start); s.obs_kfid = dp(k.obs_kfid); s.desc_start = dp(k.desc_start); s.desc = dp(k.desc);
            s.n_lm = (int)k.lm_lmid.size(); s.lm_mp = dp(k.lm_mp); s.lm_wpt = dp(k.lm_wpt);
            LoopMapOutput &o = out[b];
            const size_t n_lm = k.lm_lmid.size(), n_kp = k.kp_lmid.size();
            o.lm_status.assign(n_lm, 0); o.lm_kp.assign(n_lm, -1); o.lm_dist.assign(n_lm, 0.f); o.lm_projpx.assign(2 * n_lm, 0.f);
            o.kp_lm.assign(n_kp, -1); o.kp_dist.assign(n_kp, 0.f);
            ov2_loopmap_result &r = res[b];
            r.lm_status = o.lm_status.data(); r.lm_kp = o.lm_kp.data(); r.lm_dist = o.lm_dist.data(); r.lm_projpx = o.lm_projpx.data();
            r.kp_lm = o.kp_lm.data(); r.kp_dist = o.kp_dist.data(); r.n_matches = 0;
        }
        const int rc = ov2_loop_match_to_map_batch(ctx.get(), &mp, (int)n_items, items.data(), res.data());
        if (rc != OV2_OK) return rc;
        for (size_t b = 0; b < n_items; b++) {                      // :743-760: keypoint's map point -> local map point, a std::map
            out[b].map_previd_newid.clear();
            for (size_t i = 0; i < in[b].kp_lmid.size(); i++)
                if (out[b].kp_lm[i] >= 0) out[b].map_previd_newid.emplace(in[b].kp_lmid[i], in[b].lm_lmid[(size_t)out[b].kp_lm[i]]);
        }
        return OV2_OK;
    }

    template <class Call>
    int lckf(Order order, std::vector<Point2f> &out_px, std::vector<float> &out_resp, std::vector<uint8_t> &out_desc, Call call) const
    {
        static_assert(sizeof(Point2f) == 2 * sizeof(float), "Point2f must be two packed floats");
        // capacities: a guess first; the counts that come back are the true ones, so a second call fits whatever the first one cut
        size_t kept_cap = 1024, all_cap = order == Order::Reference ? 16384 : 0;
        std::vector<int16_t> kxy, axy;
        std::vector<uint8_t> kresp, kvalid, kdesc, aresp;
        ov2_lckf_result r = {};
        for (int attempt = 0; attempt < 2; attempt++) {
            kxy.resize(2 * kept_cap); kresp.resize(kept_cap); kvalid.resize(kept_cap); kdesc.resize(32 * kept_cap);
            axy.resize(2 * all_cap); aresp.resize(all_cap);
            r = ov2_lckf_result{};
            r.kept_xy = kxy.data(); r.kept_resp = kresp.data(); r.kept_valid = kvalid.data(); r.kept_desc = kdesc.data(); r.kept_cap = (int)kept_cap;
            r.all_xy = all_cap ? axy.data() : nullptr; r.all_resp = all_cap ? aresp.data() : nullptr; r.all_cap = (int)all_cap;
            const int rc = call(&r);
            if (rc != OV2_OK) return rc;
            const bool short_kept = (size_t)r.n_kept > kept_cap, short_all = order == Order::Reference && (size_t)r.n_all > all_cap;
            if (!short_kept && !short_all) break;
            if (short_kept) kept_cap = (size_t)r.n_kept;
            if (short_all) all_cap = (size_t)r.n_all;
        }
        const size_t nk = (size_t)r.n_kept;
        std::vector<size_t> pick;                                    // slots of the kept list, in the order asked for
        if (order == Order::Raster) {
            for (size_t i = 0; i < nk; i++) pick.push_back(i);
        } else {
            std::vector<LckfCorner> kps((size_t)r.n_all);
            for (size_t i = 0; i < kps.size(); i++) kps[i] = LckfCorner{axy[2 * i], axy[2 * i + 1], aresp[i]};
            retainBestReferenceOrder(kps, lp_.retain);
            if (kps.size() != nk) return OV2_EINVAL;                   // (cannot happen: the same set by definition)
            for (const LckfCorner &k : kps) {                          // the kept list is sorted by (y, x)
                size_t lo = 0, hi = nk;
                while (lo < hi) {
                    const size_t mid = (lo + hi) / 2;
                    if (kxy[2 * mid + 1] < k.y || (kxy[2 * mid + 1] == k.y && kxy[2 * mid] < k.x)) lo = mid + 1; else hi = mid;
                }
                if (lo >= nk || kxy[2 * lo] != k.x || kxy[2 * lo + 1] != k.y) return OV2_EINVAL;
                pick.push_back(lo);
            }
        }
        out_px.clear(); out_resp.clear(); out_desc.clear();
        for (const size_t i : pick) {                                  // runByImageBorder keeps the order of what it keeps
            if (!kvalid[i]) continue;
            out_px.emplace_back((float)kxy[2 * i], (float)kxy[2 * i + 1]);
            out_resp.push_back((float)kresp[i]);
            out_desc.insert(out_desc.end(), kdesc.begin() + 32 * (long)i, kdesc.begin() + 32 * (long)i + 32);
        }
        return OV2_OK;
    }

    struct View { const std::vector<uint8_t> *query; const std::vector<int> *vkpids; const std::vector<uint8_t> *train; const std::vector<int> *vlmids; };

    int run(Context &ctx, const View *in, size_t n_items, std::vector<std::pair<int, int>> *const *out) const
    {
        if (n_items > 0x7fffffff || kp_.desc_bytes <= 0) return OV2_EINVAL;
        const size_t nb = (size_t)kp_.desc_bytes;
        std::vector<ov2_knn_item> items(n_items);
        std::vector<ov2_knn_result> res(n_items);
        std::vector<std::vector<int>> buf(n_items);                 // idx 2n | dist 2n | pair_query n | pair_train n
        std::vector<std::vector<uint8_t>> good(n_items);
        for (size_t b = 0; b < n_items; b++) {
            const size_t nq = in[b].vkpids->size(), nt = in[b].vlmids->size();
            // the library reads desc_bytes per id: a row table of another length is the caller's error, not a read past the end
            if (in[b].query->size() != nb * nq || in[b].train->size() != nb * nt || nq > 0x7fffffff || nt > 0x7fffffff) return OV2_EINVAL;
            ov2_knn_item &s = items[b];
            s.n_query = (int)nq; s.n_train = (int)nt;
            s.query = nq ? in[b].query->data() : nullptr; s.train = nt ? in[b].train->data() : nullptr;
            buf[b].assign(6 * nq, -1); good[b].assign(nq, 0);
            ov2_knn_result &r = res[b];
            r.idx = buf[b].data(); r.dist = buf[b].data() + 2 * nq; r.pair_query = buf[b].data() + 4 * nq; r.pair_train = buf[b].data() + 5 * nq;
            r.good = good[b].data(); r.n_pairs = 0;
        }
        const int rc = ov2_knn_match_batch(ctx.get(), &kp_, (int)n_items, items.data(), res.data());
        if (rc != OV2_OK) return rc;
        for (size_t b = 0; b < n_items; b++)                        // :444-448
            for (int i = 0; i < res[b].n_pairs; i++)
                out[b]->emplace_back((*in[b].vkpids)[(size_t)res[b].pair_query[i]], (*in[b].vlmids)[(size_t)res[b].pair_train[i]]);
        return OV2_OK;
    }
};

}  // namespace ov2
