// visual_front_end.hpp -- C++ adapter for the GPU half of VisualFrontEnd (/root/reference/src/visual_front_end.cpp):
// preprocessImage (:1143-1177) + kltTracking (:132-275) on ov2_tracker_* -- ONE enqueue, ONE synchronisation per frame.
// The reference's members prev_pyr_ / cur_pyr_ live inside the tracker object; kltTracking's two fbKltTracking calls, the
// retry of lost prior tracks and the bp3preq_ rule are reproduced by the library (include/ov2slam_hip.h).
#pragma once
#include <algorithm>
#include <cmath>
#include "ov2_types.hpp"

namespace ov2 {

class FrameTracker {
public:
    // SlamParams fields of the same names (slam_params.hpp): nklt_win_size_, nklt_pyr_lvl_, nmax_iter_, fmax_px_precision_,
    // nklt_err_, fmax_fbklt_dist_, use_clahe_, fclahe_val_, nbmaxkps_
    FrameTracker(Context &ctx, int img_w, int img_h, int nklt_win_size, int nklt_pyr_lvl, int nmax_iter, float fmax_px_precision,
                 float nklt_err, float fmax_fbklt_dist, bool use_clahe, double fclahe_val, int nbmaxkps, bool use_graph = true)
    {
        ov2_tracker_config c{};
        c.w = img_w; c.h = img_h; c.win = nklt_win_size; c.nklt_pyr_lvl = nklt_pyr_lvl; c.prior_pyr_lvl = 1;
        c.max_iter = nmax_iter; c.eps = fmax_px_precision; c.err_th = nklt_err; c.fb_dist = fmax_fbklt_dist;
        c.use_clahe = use_clahe ? 1 : 0; c.clahe_clip = fclahe_val; c.tiles_x = img_w / 50; c.tiles_y = img_h / 50;   // ov2slam.cpp:85-89
        // headroom: a frame can carry more than nbmaxkps_ keypoints between keyframes (extractKeypoints tops up cells that several
        // tracked keypoints share, map_manager.cpp:74 prunes at the next keyframe only); beyond 2 x the library chunks (same results)
        c.n_max = 2 * nbmaxkps; c.use_graph = use_graph ? 1 : 0;
        if (ov2_tracker_create(ctx.get(), &c, &t_) != OV2_OK) throw std::runtime_error(std::string("ov2_tracker_create: ") + ov2_last_error());
    }
    ~FrameTracker() { ov2_tracker_destroy(t_); }              // destroy before the Context it was created on
    FrameTracker(const FrameTracker &) = delete;
    FrameTracker &operator=(const FrameTracker &) = delete;

    // pinned staging image: let the image source (ROS callback / decoder) write here to skip the host-side copy
    uint8_t *imageBuffer(int *stride) { return ov2_tracker_image_buffer(t_, stride); }

    // VisualFrontEnd::preprocessImage(img_raw): asynchronous
    bool preprocessImage(const Image8 &img_raw) { return !img_raw.empty() && ov2_tracker_preprocess(t_, img_raw.data, img_raw.step) == OV2_OK; }

    // VisualFrontEnd::kltTracking on the keypoints of pcurframe_: vkps[i] = kp.px_, vpriors[i] = projected map point for
    // keypoints with a usable 3-D prior (vhasprior[i] = 1) and kp.px_ otherwise (:160-182).  On return vpriors[i] is the
    // tracked pixel (what the reference passes to updateKeypoint), vkpstatus[i] whether the observation survives (false ->
    // removeObsFromCurFrameById, :260), bp3preq mirrors bp3preq_ (:225-230).  The reference has no error channel, so an error
    // degrades to "nothing tracked" -- and is kept: lastError() / lastErrorMessage() say why (never silent).
    void kltTracking(const std::vector<Point2f> &vkps, std::vector<Point2f> &vpriors, const std::vector<uint8_t> &vhasprior,
                     bool klt_use_prior, std::vector<bool> &vkpstatus, bool &bp3preq)
    {
        const size_t n = vkps.size();
        vkpstatus.assign(n, false);
        bp3preq = false;
        last_rc_ = OV2_OK; last_msg_.clear();
        if (n == 0) return;
        if (vpriors.size() != n || (!vhasprior.empty() && vhasprior.size() != n)) {
            last_rc_ = OV2_EINVAL; last_msg_ = "kltTracking: vkps / vpriors / vhasprior differ in length"; return;
        }
        std::vector<Point2f> out(n);
        std::vector<uint8_t> st(n, 0);
        int p3p = 0;
        const int rc = ov2_tracker_klt(t_, &vkps[0].x, &vpriors[0].x, vhasprior.empty() ? nullptr : vhasprior.data(), (int)n,
                                       klt_use_prior ? 1 : 0, &out[0].x, st.data(), &p3p);
        if (rc != OV2_OK) { last_rc_ = rc; last_msg_ = ov2_last_error(); return; }
        vpriors.swap(out);
        for (size_t i = 0; i < n; i++) vkpstatus[i] = (st[i] & 1) != 0;
        bp3preq = p3p != 0;
    }

    // preprocessImage + kltTracking in one call (one graph launch): for callers whose priors do not depend on the new image
    // (the constant-velocity motion model of the reference does not: it uses the frame time and the previous poses)
    bool trackFrame(const Image8 &img_raw, const std::vector<Point2f> &vkps, std::vector<Point2f> &vpriors, const std::vector<uint8_t> &vhasprior,
                    bool klt_use_prior, std::vector<bool> &vkpstatus, bool &bp3preq)
    {
        const size_t n = vkps.size();
        vkpstatus.assign(n, false);
        bp3preq = false;
        last_rc_ = OV2_OK; last_msg_.clear();
        if (img_raw.empty()) return false;
        if (vpriors.size() != n || (!vhasprior.empty() && vhasprior.size() != n)) {
            last_rc_ = OV2_EINVAL; last_msg_ = "trackFrame: vkps / vpriors / vhasprior differ in length"; return false;
        }
        std::vector<Point2f> out(n);
        std::vector<uint8_t> st(n, 0);
        int p3p = 0;
        const int rc = ov2_tracker_track_frame(t_, img_raw.data, img_raw.step, n ? &vkps[0].x : nullptr, n ? &vpriors[0].x : nullptr,
                                               vhasprior.empty() ? nullptr : vhasprior.data(), (int)n, klt_use_prior ? 1 : 0,
                                               n ? &out[0].x : nullptr, n ? st.data() : nullptr, &p3p);
        if (rc != OV2_OK) { last_rc_ = rc; last_msg_ = ov2_last_error(); return false; }
        if (n) vpriors.swap(out);
        for (size_t i = 0; i < n; i++) vkpstatus[i] = (st[i] & 1) != 0;
        bp3preq = p3p != 0;
        return true;
    }

    // Frame::computeKeypoint (undistorted pixel + bearing, src/frame.cpp:246-254) for every tracked position inside the per-frame
    // enqueue: call once after construction with the LEFT camera's model (CameraCalibration: K_, Dcv_, iK_), then read the results
    // of the last kltTracking / trackFrame with lastKeypoints (row-major: unpx 2 floats, bv 3 doubles per keypoint)
    bool setCalibration(int model, const double K[4], const double *D, int nD, const double iK[9])
    {
        return ov2_tracker_set_calibration(t_, model, K, D, nD, iK) == OV2_OK;
    }
    // CameraCalibration::rectifyImage (src/ov2slam.cpp:242 / :255) inside the per-frame enqueue: from this call on preprocessImage /
    // trackFrame take the RAW frame and remap it on the device before CLAHE.  map: CameraCalibration::rectMap (it must outlive its
    // use here); nullptr switches it off.  Call it right after construction, like setCalibration (the graphs are re-captured).
    bool setRectification(const ov2_rectmap *map) { return ov2_tracker_set_rectification(t_, map) == OV2_OK; }
    bool lastKeypoints(size_t n, std::vector<Point2f> &vunpx, std::vector<double> &vbv) const
    {
        vunpx.resize(n); vbv.resize(3 * n);
        return n == 0 || ov2_tracker_last_keypoints(t_, (int)n, &vunpx[0].x, vbv.data()) == OV2_OK;
    }

    // cur_pyr_ / prev_pyr_ for createKeyframe, stereo matching and the device-resident detectors (valid until the next frame)
    const ov2_pyr *curPyr() const { return ov2_tracker_cur_pyr(t_); }
    const ov2_pyr *prevPyr() const { return ov2_tracker_prev_pyr(t_); }
    // the library object, e.g. for FeatureExtractor::describeBRIEF on the raw current frame
    ov2_tracker *get() const { return t_; }

    // why the last kltTracking / trackFrame tracked nothing (OV2_OK when it did not fail)
    int lastError() const { return last_rc_; }
    const std::string &lastErrorMessage() const { return last_msg_; }

private:
    ov2_tracker *t_ = nullptr;
    int last_rc_ = OV2_OK;
    std::string last_msg_;
};

// ---- frame versus previous keyframe: computeParallax (:1066-1141), checkNewKfReq (:986-1061) and the Sampson pass over the 2-D
// keypoints of epipolar2d2dFiltering (:610-652) on ov2_parallax / ov2_kf_decision / ov2_sampson_filter_2d.  The caller hands over
// what the reference's maps hold: the current frame's keypoints in the iteration order of pcurframe_->mapkps_ (the float sums run
// in that order) and the keyframe's in any order -- the adapter sorts them by lmid, the library joins on the device.
struct KfReqParams {
    double K[4] = {0, 0, 0, 0};                               // pcalib_leftcam_: fx_, fy_, cx_, cy_
    int ncellsize = 0, nbwcells = 0, nbhcells = 0;            // Frame: ncellsize_, nbwcells_, nbhcells_
    int nbmaxkps = 0;                                         // SlamParams: nbmaxkps_, finit_parallax_, stereo_
    float finit_parallax = 0.f;
    bool stereo = false;
};
struct FrameVsKeyframe {
    std::vector<int> cur_lmid;                                // Keypoint::lmid_, px_, unpx_, bv_ (3 doubles each), is3d_
    std::vector<Point2f> cur_px, cur_unpx;
    std::vector<double> cur_bv;
    std::vector<uint8_t> cur_is3d;
    double cur_Twc[7] = {0, 0, 0, 0, 0, 0, 1};                // pcurframe_->getTwc(): [t q]
    std::vector<int> kf_lmid;                                 // pkf->mapkps_, any order
    std::vector<Point2f> kf_unpx;
    double kf_Tcw[7] = {0, 0, 0, 0, 0, 0, 1};                 // pkf->getTcw(), as held
    int cur_id = 0, kf_id = 0;                                // Frame::id_
    double cur_time = 0., kf_time = 0.;                       // Frame::img_time_
    int kf_nb3dkps = 0;                                       // pkf->nb3dkps_
    bool localba_is_on = false;                               // pslamstate_->blocalba_is_on_
    int noccupcells = -1, nb3dkps = -1;                       // pcurframe_->noccupcells_ / nb3dkps_; -1: counted on the device
};

namespace detail {
// the keyframe side in ascending lmid order (what ov2_fkf_item asks for); false when the arrays differ in length or an id repeats
// bv / bv_sorted (optional, both or none): the bearings (3 doubles each) carried along, for epipolar2d2dFiltering
inline bool sortKeyframeByLmid(const std::vector<int> &lmid, const std::vector<Point2f> &unpx, std::vector<int> &lmid_sorted,
                               std::vector<float> &unpx_sorted, const std::vector<double> *bv = nullptr,
                               std::vector<double> *bv_sorted = nullptr)
{
    const size_t m = lmid.size();
    lmid_sorted.clear(); unpx_sorted.clear();
    if (unpx.size() != m) return false;
    if ((bv != nullptr) != (bv_sorted != nullptr) || (bv && bv->size() != 3 * m)) return false;
    if (bv_sorted) bv_sorted->assign(3 * m, 0.);
    std::vector<std::pair<int, size_t>> order(m);
    for (size_t i = 0; i < m; i++) order[i] = std::make_pair(lmid[i], i);
    std::sort(order.begin(), order.end());
    lmid_sorted.resize(m); unpx_sorted.resize(2 * m);
    for (size_t i = 0; i < m; i++) {
        if (i > 0 && order[i].first == order[i - 1].first) return false;
        lmid_sorted[i] = order[i].first;
        unpx_sorted[2 * i] = unpx[order[i].second].x; unpx_sorted[2 * i + 1] = unpx[order[i].second].y;
        if (bv)
            for (int c = 0; c < 3; c++) (*bv_sorted)[3 * i + c] = (*bv)[3 * order[i].second + c];
    }
    return true;
}
struct FkfPacked { std::vector<int> kf_lmid; std::vector<float> kf_unpx; ov2_fkf_item item; };
// kf_bv / kf_bv_sorted (optional, both or none): the keyframe's bearings, sorted along with its ids
inline bool packFkf(const FrameVsKeyframe &f, FkfPacked &p, const std::vector<double> *kf_bv = nullptr,
                    std::vector<double> *kf_bv_sorted = nullptr)
{
    const size_t n = f.cur_lmid.size();
    if (f.cur_px.size() != n || f.cur_unpx.size() != n || f.cur_bv.size() != 3 * n || f.cur_is3d.size() != n) return false;
    if (!sortKeyframeByLmid(f.kf_lmid, f.kf_unpx, p.kf_lmid, p.kf_unpx, kf_bv, kf_bv_sorted)) return false;
    static const float none_f[2] = {0.f, 0.f}; static const double none_d[3] = {0., 0., 0.}; static const int none_i = 0; static const uint8_t none_b = 0;
    ov2_fkf_item &it = p.item;
    it.n_cur = (int)n;
    it.cur_lmid = n ? f.cur_lmid.data() : &none_i; it.cur_px = n ? &f.cur_px[0].x : none_f; it.cur_unpx = n ? &f.cur_unpx[0].x : none_f;
    it.cur_bv = n ? f.cur_bv.data() : none_d; it.cur_is3d = n ? f.cur_is3d.data() : &none_b; it.cur_Twc = f.cur_Twc;
    it.n_kf = (int)p.kf_lmid.size();
    it.kf_lmid = it.n_kf ? p.kf_lmid.data() : &none_i; it.kf_unpx = it.n_kf ? p.kf_unpx.data() : none_f; it.kf_Tcw = f.kf_Tcw;
    it.cur_id = f.cur_id; it.kf_id = f.kf_id; it.cur_time = f.cur_time; it.kf_time = f.kf_time; it.kf_nb3dkps = f.kf_nb3dkps;
    it.localba_is_on = f.localba_is_on ? 1 : 0; it.noccupcells = f.noccupcells; it.nb3dkps = f.nb3dkps;
    return true;
}
inline ov2_fkf_params fkfParams(const KfReqParams &k)
{
    ov2_fkf_params p{};
    for (int j = 0; j < 4; j++) p.K[j] = k.K[j];
    p.ncellsize = k.ncellsize; p.nbwcells = k.nbwcells; p.nbhcells = k.nbhcells; p.nbmaxkps = k.nbmaxkps;
    p.finit_parallax = k.finit_parallax; p.stereo = k.stereo ? 1 : 0;
    return p;
}
inline bool packFkfBatch(const std::vector<FrameVsKeyframe> &fs, std::vector<FkfPacked> &packed, std::vector<ov2_fkf_item> &items)
{
    packed.resize(fs.size()); items.resize(fs.size());
    for (size_t b = 0; b < fs.size(); b++) {
        if (!packFkf(fs[b], packed[b])) return false;
        items[b] = packed[b].item;
    }
    return true;
}
}  // namespace detail

// computeParallax(kfid, do_unrot, bmedian, b2donly) is (do_unrot, b2donly ? OV2_FKF_ONLY_2D : OV2_FKF_ALL, bmedian ? OV2_FKF_MEDIAN :
// OV2_FKF_AVG); the gate ahead of the 5-point search (:488-535) is (true, epifrom3dkps ? OV2_FKF_ONLY_3D : OV2_FKF_ALL, OV2_FKF_AVG_WIDE).
// Returns OV2_OK or the library's code (ov2_last_error() says why); OV2_EINVAL for arrays that differ in length or a repeated keyframe id.
inline int computeParallax(Context &ctx, const KfReqParams &params, const FrameVsKeyframe &f, bool do_unrot, int filter, int stat,
                           ov2_parallax_result &out)
{
    detail::FkfPacked p;
    if (!detail::packFkf(f, p)) return OV2_EINVAL;
    const ov2_fkf_params fp = detail::fkfParams(params);
    return ov2_parallax(ctx.get(), &fp, &p.item, do_unrot ? 1 : 0, filter, stat, &out);
}
inline int computeParallax(Context &ctx, const KfReqParams &params, const std::vector<FrameVsKeyframe> &fs, bool do_unrot, int filter,
                           int stat, std::vector<ov2_parallax_result> &out)
{
    std::vector<detail::FkfPacked> packed;
    std::vector<ov2_fkf_item> items;
    if (!detail::packFkfBatch(fs, packed, items)) return OV2_EINVAL;
    out.assign(fs.size(), ov2_parallax_result{});
    const ov2_fkf_params fp = detail::fkfParams(params);
    return ov2_parallax_batch(ctx.get(), &fp, (int)fs.size(), items.data(), do_unrot ? 1 : 0, filter, stat, out.data());
}

// checkNewKfReq: out.decision is its return value, out.reason says which line decided
inline int checkNewKfReq(Context &ctx, const KfReqParams &params, const FrameVsKeyframe &f, ov2_kf_decision_result &out)
{
    detail::FkfPacked p;
    if (!detail::packFkf(f, p)) return OV2_EINVAL;
    const ov2_fkf_params fp = detail::fkfParams(params);
    return ov2_kf_decision(ctx.get(), &fp, &p.item, &out);
}
inline int checkNewKfReq(Context &ctx, const KfReqParams &params, const std::vector<FrameVsKeyframe> &fs, std::vector<ov2_kf_decision_result> &out)
{
    std::vector<detail::FkfPacked> packed;
    std::vector<ov2_fkf_item> items;
    if (!detail::packFkfBatch(fs, packed, items)) return OV2_EINVAL;
    out.assign(fs.size(), ov2_kf_decision_result{});
    const ov2_fkf_params fp = detail::fkfParams(params);
    return ov2_kf_decision_batch(ctx.get(), &fp, (int)fs.size(), items.data(), out.data());
}

// the loop of :624-644: vbadkpids in the order of the current frame's keypoints (the caller removes them, :646-648); verr (optional):
// the Sampson distance per current keypoint, 0 for 3-D keypoints.  Fkfcur: computeFundamentalMat12(Tidentity, Tkfcur, K_), row-major.
inline int epipolarFilter2d(Context &ctx, const FrameVsKeyframe &f, const double Fkfcur[9], float fransac_err, std::vector<int> &vbadkpids,
                            std::vector<float> *verr = nullptr)
{
    vbadkpids.clear();
    detail::FkfPacked p;
    if (!detail::packFkf(f, p)) return OV2_EINVAL;
    const size_t n = f.cur_lmid.size();
    std::vector<float> err(n ? n : 1);
    std::vector<uint8_t> bad(n ? n : 1);
    ov2_sampson2d_result r{err.data(), bad.data(), 0};
    const int rc = ov2_sampson_filter_2d(ctx.get(), &p.item, Fkfcur, fransac_err, &r);
    if (rc != OV2_OK) return rc;
    for (size_t i = 0; i < n; i++) if (bad[i]) vbadkpids.push_back(f.cur_lmid[i]);
    if (verr) { err.resize(n); verr->swap(err); }
    return OV2_OK;
}
// one Fkfcur (9 doubles) per item in vF
inline int epipolarFilter2d(Context &ctx, const std::vector<FrameVsKeyframe> &fs, const std::vector<double> &vF, float fransac_err,
                            std::vector<std::vector<int>> &vbadkpids, std::vector<std::vector<float>> *verr = nullptr)
{
    vbadkpids.assign(fs.size(), std::vector<int>());
    if (vF.size() != 9 * fs.size()) return OV2_EINVAL;
    std::vector<detail::FkfPacked> packed;
    std::vector<ov2_fkf_item> items;
    if (!detail::packFkfBatch(fs, packed, items)) return OV2_EINVAL;
    std::vector<std::vector<float>> err(fs.size());
    std::vector<std::vector<uint8_t>> bad(fs.size());
    std::vector<ov2_sampson2d_result> rs(fs.size());
    for (size_t b = 0; b < fs.size(); b++) {
        const size_t n = fs[b].cur_lmid.size();
        err[b].resize(n ? n : 1); bad[b].resize(n ? n : 1);
        rs[b] = ov2_sampson2d_result{err[b].data(), bad[b].data(), 0};
    }
    const int rc = ov2_sampson_filter_2d_batch(ctx.get(), (int)fs.size(), items.data(), vF.data(), fransac_err, rs.data());
    if (rc != OV2_OK) return rc;
    for (size_t b = 0; b < fs.size(); b++) {
        const size_t n = fs[b].cur_lmid.size();
        for (size_t i = 0; i < n; i++) if (bad[b][i]) vbadkpids[b].push_back(fs[b].cur_lmid[i]);
        err[b].resize(n);
    }
    if (verr) verr->swap(err);
    return OV2_OK;
}

// ---- epipolar2d2dFiltering (:440-656) as one device chain on ov2_epipolar_filter: the join, the parallax gate, the 5-point search
// over a table drawn on the device from `seed`, the 50 % rule, the removals and the Sampson pass over the 2-D keypoints.  The frame is
// a FrameVsKeyframe (the current keypoints in the iteration order of pcurframe_->mapkps_, the keyframe's in any order) plus the
// keyframe's bearings and Twc.  vremove: the lmids the reference hands to removeObsFromCurFrameById, in its order -- the RANSAC
// outliers ascending in join order (:587-590), then the 2-D keypoints in array order (:646-648).  out.r.Twc_model (where
// out.r.pose_from_model) is the pose of the UNREFINED model: the reference refines it first (OpenGV, not provided), so it is the
// caller's decision whether to setTwc() with it.
struct EpipolarFilterParams {
    KfReqParams kf;                                           // K and stereo are read
    int nransac_iter = 100;                                   // SlamParams: nransac_iter_, fransac_err_, mono_
    float fransac_err = 3.f;
    bool mono = false;
    double threshold = 0.;                                    // 0: 2 (1 - cos(atan(fransac_err / focal))) from K, as the reference
    double probability = 0.99;
    int n_rows = 200;                                         // rows of the sample table per frame
};
struct EpipolarFilterInput {
    FrameVsKeyframe f;
    std::vector<double> kf_bv;                                // pkf's Keypoint::bv_, 3 doubles each, in the order of f.kf_lmid
    double kf_Twc[7] = {0, 0, 0, 0, 0, 0, 1};                 // pkf->getTwc()
    int nbkfs = 0;                                            // pmap_->nbkfs_
    unsigned long long seed = 0;
};
struct EpipolarFilterOutput {
    ov2_epifilter_result r;
    std::vector<uint8_t> removed;
    std::vector<int> pair_cur;
    std::vector<float> err;
    std::vector<int> vremove;
};
namespace detail {
struct EpifPacked { FkfPacked fkf; std::vector<double> kf_bv; ov2_epifilter_item item; };
inline bool packEpif(const EpipolarFilterInput &in, EpifPacked &p, EpipolarFilterOutput &out)
{
    const size_t n = in.f.cur_lmid.size();
    if (!packFkf(in.f, p.fkf, &in.kf_bv, &p.kf_bv)) return false;          // one sort: ids, pixels and bearings together
    static const double none_d[3] = {0., 0., 0.};
    p.item.fkf = p.fkf.item;
    p.item.kf_bv = p.kf_bv.empty() ? none_d : p.kf_bv.data();
    p.item.kf_Twc = in.kf_Twc; p.item.nbkfs = in.nbkfs; p.item.seed = in.seed;
    out.removed.assign(n ? n : 1, 0); out.pair_cur.assign(n ? n : 1, 0); out.err.assign(n ? n : 1, 0.f); out.vremove.clear();
    out.r = ov2_epifilter_result{};
    out.r.removed = out.removed.data(); out.r.pair_cur = out.pair_cur.data(); out.r.err = out.err.data();
    return true;
}
inline ov2_epifilter_params epifParams(const EpipolarFilterParams &c)
{
    ov2_epifilter_params p{};
    p.fkf = fkfParams(c.kf);
    p.epi.max_iterations = c.nransac_iter; p.epi.probability = c.probability; p.epi.boptimize = 0;
    if (c.threshold > 0.) p.epi.threshold = c.threshold;
    else {                                                    // src/multi_view_geometry.cpp:640-641
        const float focal = (float)((double)((float)c.kf.K[0] + (float)c.kf.K[1]) / 2.);
        p.epi.threshold = 2.0 * (1.0 - std::cos(std::atan((double)(c.fransac_err / focal))));
    }
    p.fransac_err = c.fransac_err; p.mono = c.mono ? 1 : 0; p.n_rows = c.n_rows;
    return p;
}
inline void finishEpif(const EpipolarFilterInput &in, EpipolarFilterOutput &out)
{
    const size_t n = in.f.cur_lmid.size();
    out.removed.resize(n); out.err.resize(n);
    out.pair_cur.resize((size_t)(out.r.m > 0 ? out.r.m : 0));
    for (int idx : out.pair_cur) if (out.removed[(size_t)idx] == 1) out.vremove.push_back(in.f.cur_lmid[(size_t)idx]);
    for (size_t i = 0; i < n; i++) if (out.removed[i] == 2) out.vremove.push_back(in.f.cur_lmid[i]);
    out.r.removed = out.removed.data(); out.r.pair_cur = out.pair_cur.data(); out.r.err = out.err.data();
}
}  // namespace detail

inline int epipolar2d2dFiltering(Context &ctx, const EpipolarFilterParams &params, const EpipolarFilterInput &in, EpipolarFilterOutput &out)
{
    detail::EpifPacked p;
    if (!detail::packEpif(in, p, out)) return OV2_EINVAL;
    const ov2_epifilter_params ep = detail::epifParams(params);
    const int rc = ov2_epipolar_filter(ctx.get(), &ep, &p.item, &out.r);
    if (rc != OV2_OK) return rc;
    detail::finishEpif(in, out);
    return OV2_OK;
}
// the frames of a lock-step batch in one chain
inline int epipolar2d2dFiltering(Context &ctx, const EpipolarFilterParams &params, const std::vector<EpipolarFilterInput> &ins,
                                 std::vector<EpipolarFilterOutput> &outs)
{
    std::vector<detail::EpifPacked> packed(ins.size());
    std::vector<ov2_epifilter_item> items(ins.size());
    std::vector<ov2_epifilter_result> rs(ins.size());
    outs.assign(ins.size(), EpipolarFilterOutput());
    for (size_t b = 0; b < ins.size(); b++) {
        if (!detail::packEpif(ins[b], packed[b], outs[b])) return OV2_EINVAL;
        items[b] = packed[b].item; rs[b] = outs[b].r;
    }
    const ov2_epifilter_params ep = detail::epifParams(params);
    const int rc = ov2_epipolar_filter_batch(ctx.get(), &ep, (int)ins.size(), items.data(), rs.data());
    if (rc != OV2_OK) return rc;
    for (size_t b = 0; b < ins.size(); b++) { outs[b].r = rs[b]; detail::finishEpif(ins[b], outs[b]); }
    return OV2_OK;
}

// ---- trackMono's un-initialised branch (:98-113) with checkReadyForInit (:855-984) as one device chain on ov2_mono_init: the count
// of 2-D keypoints, the plain median parallax, the join, the rotation-compensated parallax of :908-913, the 5-point search over a
// table drawn on the device from `seed`, the removals and the initial pose.  The frame is a FrameVsKeyframe plus the keyframe's
// bearings.  out.r.action says which return the reference takes (OV2_MINIT_RESET: breset_req_ = true; OV2_MINIT_READY: true; any other:
// false).  vremove: the lmids the reference hands to removeObsFromCurFrameById (:962-965), in its order.  out.r.Twc_init (where
// OV2_MINIT_READY) is the pose of the UNREFINED model: the reference refines it first (OpenGV, not provided; out.r.pose_refined is
// 0), so it is NOT the reference's pose until a refinement exists.
struct MonoInitParams {
    KfReqParams kf;                                           // K and finit_parallax are read
    int nransac_iter = 100;                                   // SlamParams: nransac_iter_, fransac_err_
    float fransac_err = 3.f;
    double threshold = 0.;                                    // 0: 2 (1 - cos(atan(fransac_err / focal))) from K, as the reference
    double probability = 0.99;
    int n_rows = 200;                                         // rows of the sample table per frame
    int min_2d_kps = 50;                                      // :100
};
struct MonoInitInput {
    FrameVsKeyframe f;
    std::vector<double> kf_bv;                                // pkf's Keypoint::bv_, 3 doubles each, in the order of f.kf_lmid
    unsigned long long seed = 0;
};
struct MonoInitOutput {
    ov2_mono_init_result r;
    std::vector<uint8_t> removed;
    std::vector<int> pair_cur;
    std::vector<int> vremove;
};
namespace detail {
struct MinitPacked { FkfPacked fkf; std::vector<double> kf_bv; ov2_mono_init_item item; };
inline bool packMinit(const MonoInitInput &in, MinitPacked &p, MonoInitOutput &out)
{
    const size_t n = in.f.cur_lmid.size();
    if (!packFkf(in.f, p.fkf, &in.kf_bv, &p.kf_bv)) return false;          // one sort: ids, pixels and bearings together
    static const double none_d[3] = {0., 0., 0.};
    p.item.fkf = p.fkf.item;
    p.item.kf_bv = p.kf_bv.empty() ? none_d : p.kf_bv.data();
    p.item.seed = in.seed;
    out.removed.assign(n ? n : 1, 0); out.pair_cur.assign(n ? n : 1, 0); out.vremove.clear();
    out.r = ov2_mono_init_result{};
    out.r.removed = out.removed.data(); out.r.pair_cur = out.pair_cur.data();
    return true;
}
inline ov2_mono_init_params minitParams(const MonoInitParams &c)
{
    ov2_mono_init_params p{};
    p.fkf = fkfParams(c.kf);
    p.epi.max_iterations = c.nransac_iter; p.epi.probability = c.probability; p.epi.boptimize = 0;
    if (c.threshold > 0.) p.epi.threshold = c.threshold;
    else {                                                    // src/multi_view_geometry.cpp:640-641
        const float focal = (float)((double)((float)c.kf.K[0] + (float)c.kf.K[1]) / 2.);
        p.epi.threshold = 2.0 * (1.0 - std::cos(std::atan((double)(c.fransac_err / focal))));
    }
    p.n_rows = c.n_rows; p.min_2d_kps = c.min_2d_kps;
    return p;
}
inline void finishMinit(const MonoInitInput &in, MonoInitOutput &out)
{
    out.removed.resize(in.f.cur_lmid.size());
    out.pair_cur.resize((size_t)(out.r.m > 0 ? out.r.m : 0));
    for (int idx : out.pair_cur) if (out.removed[(size_t)idx] == 1) out.vremove.push_back(in.f.cur_lmid[(size_t)idx]);
    out.r.removed = out.removed.data(); out.r.pair_cur = out.pair_cur.data();
}
}  // namespace detail

inline int checkReadyForInit(Context &ctx, const MonoInitParams &params, const MonoInitInput &in, MonoInitOutput &out)
{
    detail::MinitPacked p;
    if (!detail::packMinit(in, p, out)) return OV2_EINVAL;
    const ov2_mono_init_params mp = detail::minitParams(params);
    const int rc = ov2_mono_init(ctx.get(), &mp, &p.item, &out.r);
    if (rc != OV2_OK) return rc;
    detail::finishMinit(in, out);
    return OV2_OK;
}
// the frames of a lock-step batch in one chain
inline int checkReadyForInit(Context &ctx, const MonoInitParams &params, const std::vector<MonoInitInput> &ins, std::vector<MonoInitOutput> &outs)
{
    std::vector<detail::MinitPacked> packed(ins.size());
    std::vector<ov2_mono_init_item> items(ins.size());
    std::vector<ov2_mono_init_result> rs(ins.size());
    outs.assign(ins.size(), MonoInitOutput());
    for (size_t b = 0; b < ins.size(); b++) {
        if (!detail::packMinit(ins[b], packed[b], outs[b])) return OV2_EINVAL;
        items[b] = packed[b].item; rs[b] = outs[b].r;
    }
    const ov2_mono_init_params mp = detail::minitParams(params);
    const int rc = ov2_mono_init_batch(ctx.get(), &mp, (int)ins.size(), items.data(), rs.data());
    if (rc != OV2_OK) return rc;
    for (size_t b = 0; b < ins.size(); b++) { outs[b].r = rs[b]; detail::finishMinit(ins[b], outs[b]); }
    return OV2_OK;
}

// ---- the priors of kltTracking (:156-184) on ov2_klt_priors: every 3-D keypoint's map point projected with the predicted pose
// (projWorldToImageDist), a prior where it lands in the image (isInImage) and kp.px_ otherwise.  The caller hands over the
// keypoints in the iteration order of pcurframe_->mapkps_ with the map point of each 3-D one (pmap_->map_plms_.at(lmid)->getPoint();
// not read for 2-D keypoints) and the predicted pose inverted (Tcw = [t q]).  MotionModel itself stays with the caller.
struct KltPriorsInput {
    std::vector<Point2f> px;                                  // Keypoint::px_
    std::vector<uint8_t> is3d;                                // Keypoint::is3d_
    std::vector<double> wpt;                                  // 3 doubles per keypoint
    double Tcw[7] = {0, 0, 0, 0, 0, 0, 1};
};

namespace detail {
// false when the arrays differ in length; an empty frame gets non-NULL arrays
inline bool packKltPriors(const KltPriorsInput &f, ov2_klt_priors_item &it)
{
    const size_t n = f.px.size();
    if (f.is3d.size() != n || f.wpt.size() != 3 * n || n > 0x7fffffffu) return false;
    static const float none_f[2] = {0.f, 0.f}; static const double none_d[3] = {0., 0., 0.}; static const uint8_t none_b = 0;
    it.Tcw = f.Tcw; it.n = (int)n;
    it.px = n ? &f.px[0].x : none_f; it.is3d = n ? f.is3d.data() : &none_b; it.wpt = n ? f.wpt.data() : none_d;
    return true;
}
inline ov2_klt_priors_params kltPriorsParams(const ProjectionCamera &cam, bool klt_use_prior)
{
    ov2_klt_priors_params p{};
    p.model = cam.model;
    for (int j = 0; j < 4; j++) p.K[j] = cam.K[j];
    p.D = cam.D.empty() ? nullptr : cam.D.data(); p.nD = (int)cam.D.size();
    p.img_w = cam.img_w; p.img_h = cam.img_h; p.klt_use_prior = klt_use_prior ? 1 : 0;
    return p;
}
}  // namespace detail

// vpriors[i] / vhasprior[i] are what FrameTracker::kltTracking / trackFrame take.  Returns OV2_OK or the library's code
// (ov2_last_error() says why); OV2_EINVAL for arrays that differ in length.
inline int kltPriors(Context &ctx, const ProjectionCamera &cam, bool klt_use_prior, const KltPriorsInput &f, std::vector<Point2f> &vpriors,
                     std::vector<uint8_t> &vhasprior)
{
    ov2_klt_priors_item it{};
    if (!detail::packKltPriors(f, it)) return OV2_EINVAL;
    const size_t n = f.px.size();
    vpriors.assign(n ? n : 1, Point2f()); vhasprior.assign(n ? n : 1, 0);
    ov2_klt_priors_result r{&vpriors[0].x, vhasprior.data(), 0};
    const ov2_klt_priors_params p = detail::kltPriorsParams(cam, klt_use_prior);
    const int rc = ov2_klt_priors(ctx.get(), &p, &it, &r);
    vpriors.resize(n); vhasprior.resize(n);
    return rc;
}
// the frames of a lock-step batch in one launch
inline int kltPriors(Context &ctx, const ProjectionCamera &cam, bool klt_use_prior, const std::vector<KltPriorsInput> &fs,
                     std::vector<std::vector<Point2f>> &vpriors, std::vector<std::vector<uint8_t>> &vhasprior)
{
    const size_t B = fs.size();
    std::vector<ov2_klt_priors_item> items(B);
    std::vector<ov2_klt_priors_result> rs(B);
    vpriors.assign(B, std::vector<Point2f>()); vhasprior.assign(B, std::vector<uint8_t>());
    for (size_t b = 0; b < B; b++) {
        if (!detail::packKltPriors(fs[b], items[b])) return OV2_EINVAL;
        const size_t n = fs[b].px.size();
        vpriors[b].assign(n ? n : 1, Point2f()); vhasprior[b].assign(n ? n : 1, 0);
        rs[b] = ov2_klt_priors_result{&vpriors[b][0].x, vhasprior[b].data(), 0};
    }
    const ov2_klt_priors_params p = detail::kltPriorsParams(cam, klt_use_prior);
    const int rc = ov2_klt_priors_batch(ctx.get(), &p, (int)B, items.data(), rs.data());
    for (size_t b = 0; b < B; b++) { vpriors[b].resize(fs[b].px.size()); vhasprior[b].resize(fs[b].px.size()); }
    return rc;
}

// ---- computePose (:659-851) on ov2_compute_pose: P3P -> removal of its outliers -> ceresPnP -> the acceptance test as ONE
// device-resident chain with one synchronisation.  The caller hands over the packed arrays the reference builds at :675-712, in
// the iteration order of pcurframe_->mapkps_ over the 3-D keypoints with a live map point, and acts on the result:
//   OV2_POSE_TOO_FEW       return (:667)
//   OV2_POSE_P3P_RESET     resetFrame() (:758)
//   OV2_POSE_OK            setTwc(Twc), bp3preq_ = p3p_req_out (false), removeObsFromCurFrameById(lmid[i]) where removed[i] != 0
//   OV2_POSE_PNP_REQ_P3P   bp3preq_ = p3p_req_out (true) (:817)
//   OV2_POSE_PNP_RESET     setTwc(Twc) (P3P's, :766), remove where removed[i] == 1, then resetFrame() (:824)
//   OV2_POSE_PNP_KEEP      setTwc(Twc) (P3P's), remove where removed[i] == 1
struct ComputePoseInput {
    std::vector<double> unpx;                                 // 2 per keypoint: Keypoint::unpx_
    std::vector<double> wpt;                                  // 3 per keypoint: MapPoint::getPoint()
    std::vector<int> scale;                                   // Keypoint::scale_
    std::vector<double> bv;                                   // 3 per keypoint: Keypoint::bv_ (read only where do_p3p)
    double Twc[7] = {0, 0, 0, 0, 0, 0, 1};                    // pcurframe_->getTwc()
    bool p3p_req = false;                                     // bp3preq_
    bool do_p3p = false;                                      // bp3preq_ || pslamstate_->dop3p_
    unsigned long long seed = 0;                              // the sample table is drawn from it (see ov2::p3pRansac)
};
struct ComputePoseParams {
    int nransac_iter = 100; float fransac_err = 3.f;          // pslamstate_->nransac_iter_, fransac_err_
    float robust_mono_th = 5.9915f;
    bool apply_l2_after_robust = true, mono = false;
    float fx = 0, fy = 0, cx = 0, cy = 0;
};
struct ComputePoseOutput { ov2_pose_result r; std::vector<uint8_t> removed; };

namespace detail {
inline ov2_pose_params poseParams(const ComputePoseParams &c)
{
    ov2_pose_params p{};
    p.pnp.nmaxiter = 5; p.pnp.chi2th = (double)c.robust_mono_th; p.pnp.use_robust = 1; p.pnp.apply_l2_after_robust = c.apply_l2_after_robust ? 1 : 0;
    p.pnp.K[0] = c.fx; p.pnp.K[1] = c.fy; p.pnp.K[2] = c.cx; p.pnp.K[3] = c.cy;
    float focal = c.fx + c.fy;                                // multi_view_geometry.cpp:209-213, as ov2::p3pRansac
    focal /= 2.;
    p.p3p.mode = OV2_P3P_LMEDS; p.p3p.max_iterations = c.nransac_iter;
    p.p3p.threshold = 1.0 - std::cos(std::atan((double)(c.fransac_err / focal)));
    p.p3p.probability = 0.99; p.p3p.boptimize = 0;
    p.mono = c.mono ? 1 : 0;
    return p;
}
// false when the arrays differ in length; the sample table of a searching frame is drawn into `samples`
inline bool packPose(const ComputePoseInput &f, int nransac_iter, std::vector<int> &samples, ComputePoseOutput &out, ov2_pose_problem &it)
{
    const size_t n = f.scale.size();
    if (f.unpx.size() != 2 * n || f.wpt.size() != 3 * n || (f.do_p3p && f.bv.size() != 3 * n) || n > 0x7fffffffu) return false;
    it = ov2_pose_problem{};
    it.n = (int)n; it.unpx = f.unpx.data(); it.wpt = f.wpt.data(); it.scale = f.scale.data(); it.Twc = f.Twc;
    it.do_p3p = f.do_p3p ? 1 : 0; it.p3p_req = f.p3p_req ? 1 : 0;
    if (f.do_p3p && n >= 4) {
        const int rows = (int)std::min<long long>(2LL * std::max(nransac_iter, 0), OV2_P3P_MAX_ROWS);
        samples.assign(4 * (size_t)rows, 0);
        if (ov2_p3p_draw_samples(f.seed, (int)n, rows, samples.data()) != OV2_OK) return false;
        it.bv = f.bv.data(); it.n_rows = rows; it.samples = samples.data();
    }
    out.removed.assign(n ? n : 1, 0);
    out.r = ov2_pose_result{};
    out.r.removed = out.removed.data();
    return true;
}
}  // namespace detail

// Returns OV2_OK or the library's code (ov2_last_error() says why); OV2_EINVAL for arrays that differ in length.
inline int computePose(Context &ctx, const ComputePoseParams &params, const ComputePoseInput &f, ComputePoseOutput &out)
{
    std::vector<int> samples;
    ov2_pose_problem it;
    if (!detail::packPose(f, params.nransac_iter, samples, out, it)) return OV2_EINVAL;
    const ov2_pose_params p = detail::poseParams(params);
    const int rc = ov2_compute_pose(ctx.get(), &p, &it, &out.r);
    out.removed.resize(f.scale.size());
    out.r.removed = out.removed.data();
    return rc;
}
// the frames of a lock-step batch in one call
inline int computePose(Context &ctx, const ComputePoseParams &params, const std::vector<ComputePoseInput> &fs, std::vector<ComputePoseOutput> &out)
{
    const size_t B = fs.size();
    std::vector<std::vector<int>> samples(B);
    std::vector<ov2_pose_problem> items(B);
    std::vector<ov2_pose_result> rs(B);
    out.assign(B, ComputePoseOutput());
    for (size_t b = 0; b < B; b++) {
        if (!detail::packPose(fs[b], params.nransac_iter, samples[b], out[b], items[b])) return OV2_EINVAL;
        rs[b] = out[b].r;
    }
    const ov2_pose_params p = detail::poseParams(params);
    const int rc = ov2_compute_pose_batch(ctx.get(), &p, (int)B, items.data(), rs.data());
    for (size_t b = 0; b < B; b++) { out[b].r = rs[b]; out[b].removed.resize(fs[b].scale.size()); out[b].r.removed = out[b].removed.data(); }
    return rc;
}

// ---- MotionModel (include/visual_front_end.hpp:38-90) on ov2_motion_apply / ov2_motion_update: the reference's three methods, the
// pose as [t q] in place of a Sophus::SE3d.  The methods return the library's code; a refused call (a non-finite pose, a time that
// is not after the previous one -- where the reference exits or divides by zero) leaves the pose and the model as they were.
class MotionModel {
public:
    MotionModel() { reset(); }
    // applyMotionModel(Twc, time): Twc becomes the predicted pose; Tcw (may be NULL) its inverse, resynced (may be NULL) whether
    // prevTwc_ was moved to the caller's pose
    int applyMotionModel(Context &ctx, double Twc[7], double time, double *Tcw = nullptr, bool *resynced = nullptr)
    {
        ov2_motion_state so;
        double To[7], Ti[7];
        uint8_t rs = 0;
        const int rc = ov2_motion_apply(ctx.get(), &s_, Twc, time, &so, To, Ti, &rs);
        if (rc != OV2_OK) return rc;
        s_ = so;
        for (int k = 0; k < 7; k++) { Twc[k] = To[k]; if (Tcw) Tcw[k] = Ti[k]; }
        if (resynced) *resynced = rs != 0;
        return OV2_OK;
    }
    int updateMotionModel(Context &ctx, const double Twc[7], double time)
    {
        ov2_motion_state so;
        const int rc = ov2_motion_update(ctx.get(), &s_, Twc, time, &so);
        if (rc == OV2_OK) s_ = so;
        return rc;
    }
    void reset()
    {
        s_.prev_time = -1.;
        for (int k = 0; k < 6; k++) s_.log_relT[k] = 0.;
    }
    const ov2_motion_state &state() const { return s_; }      // prev_time_, prevTwc_, log_relT_

private:
    ov2_motion_state s_{-1., {0, 0, 0, 0, 0, 0, 1}, {0, 0, 0, 0, 0, 0}};
};

}  // namespace ov2
