// mapper.hpp -- C++ adapter for the mapper's keyframe triangulation (Mapper::triangulateStereo + Mapper::triangulateTemporal,
// src/mapper.cpp:191-461) over ov2_triangulate_keyframe[_batch].  The reference walks the map inside its loops;
// here the caller walks it once before the call (which keypoints are stereo, which map point's first observer is the temporal
// source, :243-295) and replays the returned actions afterwards, in the order the reference applies them.
#pragma once
#include <cstring>
#include "ov2_types.hpp"

namespace ov2 {

// What one keypoint asks of the map, in the reference's order: the stereo loop's actions first, then the temporal loop's.
enum class TriAction { RemoveStereoKeypoint, UpdateMapPoint, RemoveMapPointObs };
struct TriMapAction {
    TriAction op;
    int lmid;
    int kfid;             // UpdateMapPoint: the anchor keyframe (the new one for stereo points, the source for temporal ones);
                          // RemoveMapPointObs: the new keyframe (removeMapPointObs(lmid, frame.kfid_))
    double wpt[3];
    double invdepth;
};

// The new keyframe's keypoints (n = lmids.size()) and the source keyframes of its temporal candidates.  Empty is_stereo / src
// mean "none"; runpx / rbv are read for stereo keypoints, src_unpx / src_bv where src[i] >= 0.
struct TriKeyframeInput {
    int kfid = 0;
    double Twc[7] = {0, 0, 0, 0, 0, 0, 1};
    std::vector<int> lmids;
    std::vector<Point2f> unpx;          // n
    std::vector<double> bv;             // 3n
    std::vector<uint8_t> is_stereo;     // n or empty: is_stereo_ && !is3d_
    std::vector<Point2f> runpx;         // n or empty
    std::vector<double> rbv;            // 3n or empty
    std::vector<int> src;               // n or empty: row of the source table, -1 = not a temporal candidate
    std::vector<Point2f> src_unpx;      // n or empty: the source keyframe's keypoint of the same map point
    std::vector<double> src_bv;         // 3n or empty
    std::vector<int> src_kfid;          // m: the source keyframes' ids
    std::vector<double> src_Twc, src_Tcw;   // 7m each, as held
};

struct TriKeyframeOutput {
    std::vector<uint8_t> status;        // n: OV2_TRI_* bits
    std::vector<double> wpt, invdepth;  // 3n, n
    std::vector<TriMapAction> actions;
    int n_stereo = 0, n_stereo_good = 0, n_candidates = 0, n_temporal_good = 0;
};

class Mapper {
public:
    // calibration and settings: left K / iK_, right K, getExtrinsic() (Tc0ci_) and Tcic0_ of the right camera, as held
    Mapper(bool stereo, bool rect, float fmax_reproj_err, const double K[4], const double iK[9], const double Kr[4],
           const double Tlr[7], const double Tcic0[7])
    {
        std::memset(&p_, 0, sizeof(p_));
        p_.stereo = stereo ? 1 : 0; p_.rect = rect ? 1 : 0; p_.fmax_reproj_err = fmax_reproj_err;
        std::memcpy(p_.K, K, sizeof(p_.K)); std::memcpy(p_.iK, iK, sizeof(p_.iK)); std::memcpy(p_.Kr, Kr, sizeof(p_.Kr));
        std::memcpy(p_.Tlr, Tlr, sizeof(p_.Tlr)); std::memcpy(p_.Tcic0, Tcic0, sizeof(p_.Tcic0));
    }
    const ov2_tri_params &params() const { return p_; }

    // triangulateStereo + triangulateTemporal of one keyframe (one launch, one synchronisation); OV2_OK or the library's error
    int triangulate(Context &ctx, const TriKeyframeInput &in, TriKeyframeOutput &out) const
    {
        std::vector<TriKeyframeOutput> o(1);
        const int rc = run(ctx, &in, 1, o.data());
        if (rc == OV2_OK) out = std::move(o[0]);
        return rc;
    }
    // the keyframes of a lock-step batch in one launch
    int triangulateBatch(Context &ctx, const std::vector<TriKeyframeInput> &in, std::vector<TriKeyframeOutput> &out) const
    {
        std::vector<TriKeyframeOutput> o(in.size());
        const int rc = run(ctx, in.data(), in.size(), o.data());
        if (rc == OV2_OK) out = std::move(o);
        return rc;
    }

private:
    ov2_tri_params p_;

    static const float *fp(const std::vector<Point2f> &v) { return v.empty() ? nullptr : &v[0].x; }
    template <class T> static const T *dp(const std::vector<T> &v) { return v.empty() ? nullptr : v.data(); }

    static bool sizes_ok(const TriKeyframeInput &k)
    {
        const size_t n = k.lmids.size(), m = k.src_kfid.size();
        auto opt = [](size_t s, size_t want) { return s == 0 || s == want; };
        return k.unpx.size() == n && k.bv.size() == 3 * n && opt(k.is_stereo.size(), n) && opt(k.runpx.size(), n) &&
               opt(k.rbv.size(), 3 * n) && opt(k.src.size(), n) && opt(k.src_unpx.size(), n) && opt(k.src_bv.size(), 3 * n) &&
               k.src_Twc.size() == 7 * m && k.src_Tcw.size() == 7 * m && n <= 0x7fffffff;
    }

    int run(Context &ctx, const TriKeyframeInput *in, size_t n_items, TriKeyframeOutput *out) const
    {
        if (n_items > 0x7fffffff) return OV2_EINVAL;
        std::vector<ov2_tri_keyframe> kfs(n_items);
        std::vector<ov2_tri_result> res(n_items);
        for (size_t b = 0; b < n_items; b++) {
            const TriKeyframeInput &k = in[b];
            if (!sizes_ok(k)) return OV2_EINVAL;
            const size_t n = k.lmids.size();
            ov2_tri_keyframe &s = kfs[b];
            s.n = (int)n; s.Twc = k.Twc; s.unpx = fp(k.unpx); s.bv = dp(k.bv); s.is_stereo = dp(k.is_stereo);
            s.runpx = fp(k.runpx); s.rbv = dp(k.rbv); s.src = dp(k.src); s.src_unpx = fp(k.src_unpx); s.src_bv = dp(k.src_bv);
            s.n_src = (int)k.src_kfid.size(); s.src_Twc = dp(k.src_Twc); s.src_Tcw = dp(k.src_Tcw);
            TriKeyframeOutput &o = out[b];
            o.status.assign(n, 0); o.wpt.assign(3 * n, 0.); o.invdepth.assign(n, 0.);
            res[b].status = o.status.data(); res[b].wpt = o.wpt.data(); res[b].invdepth = o.invdepth.data();
        }
        const int rc = ov2_triangulate_keyframe_batch(ctx.get(), &p_, (int)n_items, kfs.data(), res.data());
        if (rc != OV2_OK) return rc;
        for (size_t b = 0; b < n_items; b++) {
            const TriKeyframeInput &k = in[b];
            TriKeyframeOutput &o = out[b];
            o.n_stereo = res[b].n_stereo; o.n_stereo_good = res[b].n_stereo_good;
            o.n_candidates = res[b].n_candidates; o.n_temporal_good = res[b].n_temporal_good;
            o.actions.clear();
            const size_t n = k.lmids.size();
            for (size_t i = 0; i < n; i++) {                       // triangulateStereo's loop (:398-456)
                const uint8_t s = o.status[i];
                if (!(s & OV2_TRI_STEREO_TRIED)) continue;
                if (s & OV2_TRI_STEREO_OK) o.actions.push_back(update(k.lmids[i], k.kfid, &o.wpt[3 * i], o.invdepth[i]));
                else o.actions.push_back(TriMapAction{TriAction::RemoveStereoKeypoint, k.lmids[i], k.kfid, {0, 0, 0}, 0.});
            }
            for (size_t i = 0; i < n; i++) {                       // triangulateTemporal's loop (:241-337)
                const uint8_t s = o.status[i];
                if (s & OV2_TRI_TEMPORAL_OK) o.actions.push_back(update(k.lmids[i], k.src_kfid[(size_t)k.src[i]], &o.wpt[3 * i], o.invdepth[i]));
                else if (s & OV2_TRI_REMOVE_OBS) o.actions.push_back(TriMapAction{TriAction::RemoveMapPointObs, k.lmids[i], k.kfid, {0, 0, 0}, 0.});
            }
        }
        return OV2_OK;
    }

    static TriMapAction update(int lmid, int kfid, const double *w, double inv)
    {
        return TriMapAction{TriAction::UpdateMapPoint, lmid, kfid, {w[0], w[1], w[2]}, inv};
    }
};

}  // namespace ov2
