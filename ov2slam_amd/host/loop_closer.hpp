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
#pragma once
#include <algorithm>
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

private:
    ov2_knn_params kp_ = {};
    ov2_lckf_params lp_ = {20, 300, 2};

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
