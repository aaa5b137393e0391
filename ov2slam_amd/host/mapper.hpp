// mapper.hpp -- C++ adapter for the mapper's keyframe triangulation (Mapper::triangulateStereo + Mapper::triangulateTemporal,
// src/mapper.cpp:191-461) over ov2_triangulate_keyframe[_batch].  The reference walks the map inside its loops;
// here the caller walks it once before the call (which keypoints are stereo, which map point's first observer is the temporal
// source, :243-295) and replays the returned actions afterwards, in the order the reference applies them.
// The same for the local-map matching (Mapper::matchToMap, :576-774) over ov2_match_to_map[_batch]: the caller flattens the local
// map and the keyframe's keypoints (MatchKeyframeInput) and gets map_previd_newid back, ready for mergeMatches.
#pragma once
#include <cmath>
#include <cstring>
#include <map>
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

// Mapper::matchToMap: the arrays of ov2_match_keyframe (include/ov2slam_hip.h) plus the ids the rows stand for.
struct MatchKeyframeInput {
    double Tcw[7] = {0, 0, 0, 0, 0, 0, 1};
    int nb3dkps = 0;
    std::vector<int> kp_lmid;           // n_kp: the keypoints' lmid_ (the keys of map_previd_newid)
    std::vector<Point2f> kp_px;         // n_kp
    std::vector<int> kp_mp;             // n_kp: row of the map-point table, -1 = no usable map point
    std::vector<int> cell_start, cell_kp;   // ncells + 1 offsets; keypoint rows per cell in vgridkps_ order
    std::vector<int> obs_start;         // n_mp + 1
    std::vector<int> obs_kfid, obs_kf;  // per observation: keyframe id (ascending inside a row); row of the pose table, -1 = stale
    std::vector<Point2f> obs_px;        // per observation
    std::vector<int> desc_start;        // n_mp + 1
    std::vector<uint8_t> desc;          // 32 per descriptor
    std::vector<double> kf_Tcw;         // 7 per pose row, as held
    std::vector<int> lm_lmid;           // n_lm: the local map points' ids, in iteration order (the values of map_previd_newid)
    std::vector<int> lm_mp;             // n_lm: row of the map-point table
    std::vector<double> lm_wpt;         // 3 n_lm
};

struct MatchKeyframeOutput {
    std::vector<uint8_t> lm_status;     // n_lm: OV2_MATCH_* bits
    std::vector<int> lm_kp;             // n_lm: proposed keypoint row or -1
    std::vector<float> lm_dist, lm_projpx;   // n_lm, 2 n_lm
    std::vector<int> kp_lm;             // n_kp: winning local-map index or -1
    std::vector<float> kp_dist;         // n_kp
    std::map<int, int> map_previd_newid;    // keypoint's lmid -> local map point's lmid
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

    // what matchToMap needs beyond the triangulation's settings: the left camera's model (OV2_CAM_*) / K / distortion vector / image
    // size, Frame::ncellsize_, and the SlamParams' fmax_proj_pxdist_ / fmax_desc_dist_
    void setMatching(int model, const double K[4], const double *D, int nD, double img_w, double img_h, int ncellsize,
                     float fmax_proj_pxdist, float fmax_desc_dist)
    {
        std::memset(&mp_, 0, sizeof(mp_));
        mp_.model = model; std::memcpy(mp_.K, K, sizeof(mp_.K));
        md_.assign(D, D + (nD > 0 ? nD : 0));
        mp_.nD = nD; mp_.img_w = img_w; mp_.img_h = img_h; mp_.ncellsize = ncellsize;
        mp_.fmax_proj_pxdist = fmax_proj_pxdist; mp_.fmax_desc_dist = fmax_desc_dist; mp_.desc_bytes = 32;
        has_match_ = true;
    }
    // Mapper::matchToMap of one keyframe (one upload, one synchronisation); OV2_OK or the library's error
    int matchToMap(Context &ctx, const MatchKeyframeInput &in, MatchKeyframeOutput &out) const
    {
        std::vector<MatchKeyframeOutput> o(1);
        const int rc = runMatch(ctx, &in, 1, o.data());
        if (rc == OV2_OK) out = std::move(o[0]);
        return rc;
    }
    // the keyframes of a lock-step batch in one call
    int matchToMapBatch(Context &ctx, const std::vector<MatchKeyframeInput> &in, std::vector<MatchKeyframeOutput> &out) const
    {
        std::vector<MatchKeyframeOutput> o(in.size());
        const int rc = runMatch(ctx, in.data(), in.size(), o.data());
        if (rc == OV2_OK) out = std::move(o);
        return rc;
    }

private:
    ov2_tri_params p_;
    ov2_match_params mp_ = {};
    std::vector<double> md_;
    bool has_match_ = false;

    static bool match_sizes_ok(const MatchKeyframeInput &k)
    {
        const size_t n_kp = k.kp_lmid.size(), n_lm = k.lm_lmid.size();
        if (k.kp_px.size() != n_kp || k.kp_mp.size() != n_kp || k.lm_mp.size() != n_lm || k.lm_wpt.size() != 3 * n_lm) return false;
        if (k.obs_start.size() != k.desc_start.size() || k.kf_Tcw.size() % 7) return false;
        if (!k.obs_start.empty() && (k.obs_start.back() < 0 || k.desc_start.back() < 0)) return false;
        const size_t n_ob = k.obs_start.empty() ? 0 : (size_t)k.obs_start.back(), n_de = k.desc_start.empty() ? 0 : (size_t)k.desc_start.back();
        if (k.obs_kfid.size() != n_ob || k.obs_kf.size() != n_ob || k.obs_px.size() != n_ob || k.desc.size() != 32 * n_de) return false;
        if (!k.cell_start.empty() && (k.cell_start.back() < 0 || k.cell_kp.size() != (size_t)k.cell_start.back())) return false;
        return n_kp <= 0x7fffffff && n_lm <= 0x7fffffff && k.obs_start.size() <= 0x7fffffff && k.kf_Tcw.size() / 7 <= 0x7fffffff;
    }

    int runMatch(Context &ctx, const MatchKeyframeInput *in, size_t n_items, MatchKeyframeOutput *out) const
    {
        if (!has_match_ || n_items > 0x7fffffff) return OV2_EINVAL;
        ov2_match_params mp = mp_;
        mp.D = md_.empty() ? nullptr : md_.data();
        std::vector<ov2_match_keyframe> kfs(n_items);
        std::vector<ov2_match_result> res(n_items);
        for (size_t b = 0; b < n_items; b++) {
            const MatchKeyframeInput &k = in[b];
            if (!match_sizes_ok(k)) return OV2_EINVAL;
            // the library reads ncells + 1 offsets: a cell table of another length is the caller's error, not a read past the end
            const size_t nbw = (size_t)std::ceil((float)mp.img_w / (float)mp.ncellsize), nbh = (size_t)std::ceil((float)mp.img_h / (float)mp.ncellsize);
            if (!k.cell_start.empty() && k.cell_start.size() != nbw * nbh + 1) return OV2_EINVAL;
            if (k.cell_start.empty() && !k.kp_lmid.empty()) return OV2_EINVAL;
            ov2_match_keyframe &s = kfs[b];
            s.Tcw = k.Tcw; s.nb3dkps = k.nb3dkps;
            s.n_kp = (int)k.kp_lmid.size(); s.kp_px = fp(k.kp_px); s.kp_mp = dp(k.kp_mp);
            s.cell_start = dp(k.cell_start); s.cell_kp = dp(k.cell_kp);
            s.n_mp = k.obs_start.empty() ? 0 : (int)k.obs_start.size() - 1;
            s.obs_start = dp(k.obs_start); s.obs_kfid = dp(k.obs_kfid); s.obs_kf = dp(k.obs_kf); s.obs_px = fp(k.obs_px);
            s.desc_start = dp(k.desc_start); s.desc = dp(k.desc);
            s.n_kf = (int)(k.kf_Tcw.size() / 7); s.kf_Tcw = dp(k.kf_Tcw);
            s.n_lm = (int)k.lm_lmid.size(); s.lm_mp = dp(k.lm_mp); s.lm_wpt = dp(k.lm_wpt);
            MatchKeyframeOutput &o = out[b];
            const size_t n_lm = k.lm_lmid.size(), n_kp = k.kp_lmid.size();
            o.lm_status.assign(n_lm, 0); o.lm_kp.assign(n_lm, -1); o.lm_dist.assign(n_lm, 0.f); o.lm_projpx.assign(2 * n_lm, 0.f);
            o.kp_lm.assign(n_kp, -1); o.kp_dist.assign(n_kp, 0.f);
            ov2_match_result &r = res[b];
            r.lm_status = o.lm_status.data(); r.lm_kp = o.lm_kp.data(); r.lm_dist = o.lm_dist.data(); r.lm_projpx = o.lm_projpx.data();
            r.kp_lm = o.kp_lm.data(); r.kp_dist = o.kp_dist.data(); r.n_matches = 0;
        }
        const int rc = ov2_match_to_map_batch(ctx.get(), &mp, (int)n_items, kfs.data(), res.data());
        if (rc != OV2_OK) return rc;
        for (size_t b = 0; b < n_items; b++) {                      // :754-771: keypoint's map point -> local map point
            out[b].map_previd_newid.clear();
            for (size_t i = 0; i < in[b].kp_lmid.size(); i++)
                if (out[b].kp_lm[i] >= 0) out[b].map_previd_newid.emplace(in[b].kp_lmid[i], in[b].lm_lmid[(size_t)out[b].kp_lm[i]]);
        }
        return OV2_OK;
    }

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
