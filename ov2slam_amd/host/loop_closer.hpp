// loop_closer.hpp -- C++ adapter for the loop closer's descriptor matching (LoopCloser::knnMatching, src/loop_closer.cpp:378-459)
// over ov2_knn_match[_batch].  The reference walks the two frames inside the function (:391-420): which keypoints of the new
// keyframe the candidate already observes, and which map points carry a descriptor.  Here the caller does those two walks and
// hands over what they collect: the query rows with their vkpids, the train rows with their vlmids.  The call appends
// (vkpids[q], vlmids[t]) of the good rows to vkplmids in query order, exactly what :444-448 appends.
#pragma once
#include "ov2_types.hpp"

namespace ov2 {

// one query / train pair of the batch form: descriptor rows of 32 bytes, one id per row
struct KnnMatchingInput {
    std::vector<uint8_t> query; std::vector<int> vkpids;
    std::vector<uint8_t> train; std::vector<int> vlmids;
};

class LoopCloser {
public:
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

private:
    ov2_knn_params kp_ = {};
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
