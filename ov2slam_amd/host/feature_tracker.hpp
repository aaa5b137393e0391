// feature_tracker.hpp -- C++ adapter with the signature of the reference's FeatureTracker
// (/root/reference/include/feature_tracker.hpp:36-56, src/feature_tracker.cpp:35-137), forwarding to
// the C ABI.  Same argument meaning, same in/out conventions, same failure behaviour: any library
// error degrades to "nothing tracked" (all status false), never an exception.
#pragma once
#include "ov2_types.hpp"

namespace ov2 {

class FeatureTracker {
public:
    // reference: FeatureTracker(int nmax_iter, float fmax_px_precision, cv::Ptr<cv::CLAHE> pclahe)
    FeatureTracker(int nmax_iter, float fmax_px_precision) : nmax_iter_(nmax_iter), fmax_px_precision_(fmax_px_precision) {}

    // reference: void fbKltTracking(const std::vector<cv::Mat> &vprevpyr, const std::vector<cv::Mat> &vcurpyr,
    //                int nwinsize, int nbpyrlvl, float ferr, float fmax_fbklt_dist, std::vector<cv::Point2f> &vkps,
    //                std::vector<cv::Point2f> &vpriorkps, std::vector<bool> &vkpstatus) const
    // `ctx` is the calling thread's context (the method is const and is called concurrently from the
    // SLAM thread and the mapper thread: src/visual_front_end.cpp:196 / src/map_manager.cpp:510).
    void fbKltTracking(Context &ctx, const Pyramid &vprevpyr, const Pyramid &vcurpyr, int nwinsize, int nbpyrlvl,
                       float ferr, float fmax_fbklt_dist, std::vector<Point2f> &vkps, std::vector<Point2f> &vpriorkps,
                       std::vector<bool> &vkpstatus) const
    {
        fbKltTracking(ctx, vprevpyr.get(), vcurpyr.get(), nwinsize, nbpyrlvl, ferr, fmax_fbklt_dist, vkps, vpriorkps, vkpstatus);
    }
    // the same on raw handles (e.g. prev = SlamGpu::kf_front, cur = FrameTracker::curPyr(): VisualFrontEnd::kltTrackingFromKF,
    // src/visual_front_end.cpp:363, :409)
    void fbKltTracking(Context &ctx, const ov2_pyr *vprevpyr, const ov2_pyr *vcurpyr, int nwinsize, int nbpyrlvl,
                       float ferr, float fmax_fbklt_dist, std::vector<Point2f> &vkps, std::vector<Point2f> &vpriorkps,
                       std::vector<bool> &vkpstatus) const
    {
        if (vkps.empty()) return;                                   // :43-46
        const size_t n = vkps.size();
        vkpstatus.reserve(vkpstatus.size() + n);
        std::vector<uint8_t> st(n, 0);
        std::vector<Point2f> priors(vpriorkps);
        const int rc = ov2_fb_klt(ctx.get(), vprevpyr, vcurpyr, nwinsize, nbpyrlvl, nmax_iter_, fmax_px_precision_,
                                  ferr, fmax_fbklt_dist, &vkps[0].x, &priors[0].x, (int)n, st.data(), nullptr);
        if (rc == OV2_OK) vpriorkps.swap(priors);
        for (size_t i = 0; i < n; i++) vkpstatus.push_back(rc == OV2_OK && st[i] != 0);
    }

    // reference: void getLineMinSAD(const cv::Mat &iml, const cv::Mat &imr, const cv::Point2f &pt, const int nwinsize,
    //                float &xprior, float &l1err, bool bgoleft) const                              (:138-206)
    // -- here for a whole vector of points on pyramid level `level` in one launch (the reference loops over the
    // keypoints and calls it per point, src/map_manager.cpp:421-439).  xprior[i] = -1 when nothing qualified.
    void getLineMinSAD(Context &ctx, const Pyramid &leftpyr, const Pyramid &rightpyr, int level, const std::vector<Point2f> &vpts,
                       int nwinsize, std::vector<float> &vxprior, std::vector<float> &vl1err, bool bgoleft) const
    {
        vxprior.assign(vpts.size(), -1.f);
        vl1err.assign(vpts.size(), 255.f);
        if (vpts.empty()) return;
        const int rc = ov2_line_min_sad(ctx.get(), leftpyr.get(), rightpyr.get(), level, nwinsize, bgoleft ? 1 : 0, &vpts[0].x,
                                        (int)vpts.size(), vxprior.data(), vl1err.data());
        if (rc != OV2_OK) vxprior.assign(vpts.size(), -1.f);       // degrade to "no prior", like an early return
    }

    // MapManager::stereoMatching's data path (src/map_manager.cpp:367-611) for the keypoints of a keyframe in ONE enqueue and ONE
    // synchronisation (ov2_stereo_match): SAD priors on the coarsest level (rectified pairs), both fbKltTracking calls with the
    // retry of the failed 3-D-prior tracks, the epipolar gate.  vpriors3d[i] / vhasprior3d[i]: the projected map point of
    // keypoint i where one exists (:402-413, :468-480).  On return vstereo_ok[i] decides updateKeypointStereo(id, vrightkps[i]).
    // rmodel / rK / rD: the RIGHT camera (OV2_CAM_PINHOLE / OV2_CAM_FISHEYE, fx fy cx cy, distortion).
    void stereoMatching(Context &ctx, const ov2_pyr *leftpyr, const ov2_pyr *rightpyr, int nklt_win_size, int nklt_pyr_lvl, float nklt_err,
                        float fmax_fbklt_dist, bool rect, const double *Frl, int rmodel, const double rK[4], const std::vector<double> &rD,
                        const std::vector<Point2f> &vleftkps, const std::vector<Point2f> &vleftunpx, const std::vector<Point2f> &vpriors3d,
                        const std::vector<uint8_t> &vhasprior3d, std::vector<Point2f> &vrightkps, std::vector<bool> &vstereo_ok) const
    {
        const size_t n = vleftkps.size();
        vrightkps.assign(n, Point2f());
        vstereo_ok.assign(n, false);
        if (n == 0) return;
        std::vector<uint8_t> ok(n, 0);
        const bool pri = vpriors3d.size() == n && vhasprior3d.size() == n;
        const int rc = ov2_stereo_match(ctx.get(), leftpyr, rightpyr, nklt_win_size, nklt_pyr_lvl, nmax_iter_, fmax_px_precision_, nklt_err,
                                        fmax_fbklt_dist, rect ? 1 : 0, Frl, rmodel, rK, rD.empty() ? nullptr : rD.data(), (int)rD.size(),
                                        &vleftkps[0].x, &vleftunpx[0].x, pri ? &vpriors3d[0].x : nullptr, pri ? vhasprior3d.data() : nullptr,
                                        (int)n, &vrightkps[0].x, ok.data());
        if (rc != OV2_OK) return;                                   // degrade to "no stereo observation"
        for (size_t i = 0; i < n; i++) vstereo_ok[i] = ok[i] != 0;
    }

    // reference: bool inBorder(const cv::Point2f &pt, const cv::Mat &im) const  (:216-221)
    bool inBorder(const Point2f &pt, int cols, int rows) const
    {
        const float BORDER_SIZE = 1.f;
        return BORDER_SIZE <= pt.x && pt.x < cols - BORDER_SIZE && BORDER_SIZE <= pt.y && pt.y < rows - BORDER_SIZE;
    }

private:
    int nmax_iter_;
    float fmax_px_precision_;
};

// ---- the priors of MapManager::stereoMatching (src/map_manager.cpp:396-489) on ov2_stereo_priors: the map point projected into the
// right image, and without rectification the depth of the 3-D neighbours (Frame::getSurroundingKeypoints).  The caller hands over the
// keyframe's keypoints (vleftkps order) with `state` 0 = 2-D, 1 = 3-D with its map point in wpt, 2 = 3-D whose map point is gone
// (the caller does removeMapPointObs for the keypoints that come back with vskip), and vgridkps_ as rows into those arrays.
struct StereoPriorsInput {
    std::vector<Point2f> px, unpx;                            // Keypoint::px_, unpx_
    std::vector<double> bv;                                   // 3 per keypoint: bv_
    std::vector<double> wpt;                                  // 3 per keypoint: getMapPoint(lmid)->getPoint() where state == 1
    std::vector<uint8_t> state;
    std::vector<std::vector<int>> grid;                       // Frame::vgridkps_: per cell the keypoint ROWS, in the cell's order
    double Tcw[7] = {0, 0, 0, 0, 0, 0, 1};                    // frame.getTcw(), as held
};
struct StereoPriorsParams {
    ProjectionCamera rightcam;                                // pcalib_rightcam_
    double Tcic0[7] = {0, 0, 0, 0, 0, 0, 1};                  // pcalib_rightcam_->Tcic0_
    int ncellsize = 0;                                        // Frame::ncellsize_
    bool rect = false;                                        // SlamParams::bdo_stereo_rect_
};

namespace detail {
// Frame's grid size (frame.cpp:41-43): cells of ncellsize over img_w x img_h, in float; 0 for a size that has none
inline size_t priorGridCells(double img_w, double img_h, int ncellsize)
{
    if (!(img_w > 0 && img_h > 0) || ncellsize <= 0 || img_w > 65536 || img_h > 65536) return 0;
    const float c = (float)ncellsize;
    const float w = (float)img_w / c, h = (float)img_h / c;
    const size_t nbw = (size_t)w + ((float)(size_t)w < w ? 1 : 0), nbh = (size_t)h + ((float)(size_t)h < h ? 1 : 0);
    return nbw * nbh;
}
// vgridkps_ -> the offsets and rows of ov2_stereo_priors_item; false for a grid of another size than ncells or a row outside [0, n)
inline bool buildCellTable(const std::vector<std::vector<int>> &grid, size_t ncells, size_t n, std::vector<int> &cell_start,
                           std::vector<int> &cell_kp)
{
    cell_start.clear(); cell_kp.clear();
    if (grid.size() != ncells) return false;
    cell_start.reserve(ncells + 1);
    cell_start.push_back(0);
    for (const std::vector<int> &cell : grid) {
        for (int k : cell) {
            if (k < 0 || (size_t)k >= n) return false;
            cell_kp.push_back(k);
        }
        if (cell_kp.size() > 0x7fffffffu) return false;
        cell_start.push_back((int)cell_kp.size());
    }
    return true;
}
struct StereoPriorsPacked { std::vector<int> cell_start, cell_kp; ov2_stereo_priors_item item; };
inline bool packStereoPriors(const StereoPriorsParams &P, const StereoPriorsInput &f, StereoPriorsPacked &p)
{
    const size_t n = f.px.size();
    if (f.unpx.size() != n || f.bv.size() != 3 * n || f.wpt.size() != 3 * n || f.state.size() != n || n > 0x7fffffffu) return false;
    const size_t ncells = priorGridCells(P.rightcam.img_w, P.rightcam.img_h, P.ncellsize);
    if (f.grid.empty() && P.rect) { p.cell_start.assign(ncells + 1, 0); p.cell_kp.clear(); }      // not read for rectified pairs
    else if (!buildCellTable(f.grid, ncells, n, p.cell_start, p.cell_kp)) return false;
    static const float none_f[2] = {0.f, 0.f}; static const double none_d[3] = {0., 0., 0.}; static const uint8_t none_b = 0; static const int none_i = 0;
    ov2_stereo_priors_item &it = p.item;
    it.Tcw = f.Tcw; it.n = (int)n;
    it.px = n ? &f.px[0].x : none_f; it.unpx = n ? &f.unpx[0].x : none_f; it.bv = n ? f.bv.data() : none_d; it.wpt = n ? f.wpt.data() : none_d;
    it.state = n ? f.state.data() : &none_b;
    it.cell_start = p.cell_start.data(); it.cell_kp = p.cell_kp.empty() ? &none_i : p.cell_kp.data();
    return true;
}
inline ov2_stereo_priors_params stereoPriorsParams(const StereoPriorsParams &P)
{
    ov2_stereo_priors_params p{};
    p.model = P.rightcam.model;
    for (int j = 0; j < 4; j++) p.K[j] = P.rightcam.K[j];
    p.D = P.rightcam.D.empty() ? nullptr : P.rightcam.D.data(); p.nD = (int)P.rightcam.D.size();
    p.img_w = P.rightcam.img_w; p.img_h = P.rightcam.img_h;
    for (int j = 0; j < 7; j++) p.Tcic0[j] = P.Tcic0[j];
    p.ncellsize = P.ncellsize; p.rect = P.rect ? 1 : 0;
    return p;
}
}  // namespace detail

// vpriors3d / vhasprior3d are exactly what FeatureTracker::stereoMatching takes (non-zero: a prior; 1 from the map point, 2 from the
// neighbours); vskip[i]: the reference drops keypoint i from the matching (:415-418).  Returns OV2_OK or the library's code;
// OV2_EINVAL for arrays that differ in length, a grid of the wrong size or a row outside the keypoints.
inline int stereoPriors(Context &ctx, const StereoPriorsParams &P, const StereoPriorsInput &f, std::vector<Point2f> &vpriors3d,
                        std::vector<uint8_t> &vhasprior3d, std::vector<uint8_t> &vskip)
{
    detail::StereoPriorsPacked p;
    if (!detail::packStereoPriors(P, f, p)) return OV2_EINVAL;
    const size_t n = f.px.size();
    vpriors3d.assign(n ? n : 1, Point2f()); vhasprior3d.assign(n ? n : 1, 0); vskip.assign(n ? n : 1, 0);
    ov2_stereo_priors_result r{&vpriors3d[0].x, vhasprior3d.data(), vskip.data(), 0, 0, 0};
    const ov2_stereo_priors_params sp = detail::stereoPriorsParams(P);
    const int rc = ov2_stereo_priors(ctx.get(), &sp, &p.item, &r);
    vpriors3d.resize(n); vhasprior3d.resize(n); vskip.resize(n);
    return rc;
}
// the keyframes of a lock-step batch in one launch
inline int stereoPriors(Context &ctx, const StereoPriorsParams &P, const std::vector<StereoPriorsInput> &fs,
                        std::vector<std::vector<Point2f>> &vpriors3d, std::vector<std::vector<uint8_t>> &vhasprior3d,
                        std::vector<std::vector<uint8_t>> &vskip)
{
    const size_t B = fs.size();
    std::vector<detail::StereoPriorsPacked> packed(B);
    std::vector<ov2_stereo_priors_item> items(B);
    std::vector<ov2_stereo_priors_result> rs(B);
    vpriors3d.assign(B, std::vector<Point2f>()); vhasprior3d.assign(B, std::vector<uint8_t>()); vskip.assign(B, std::vector<uint8_t>());
    for (size_t b = 0; b < B; b++) {
        if (!detail::packStereoPriors(P, fs[b], packed[b])) return OV2_EINVAL;
        items[b] = packed[b].item;
        const size_t n = fs[b].px.size();
        vpriors3d[b].assign(n ? n : 1, Point2f()); vhasprior3d[b].assign(n ? n : 1, 0); vskip[b].assign(n ? n : 1, 0);
        rs[b] = ov2_stereo_priors_result{&vpriors3d[b][0].x, vhasprior3d[b].data(), vskip[b].data(), 0, 0, 0};
    }
    const ov2_stereo_priors_params sp = detail::stereoPriorsParams(P);
    const int rc = ov2_stereo_priors_batch(ctx.get(), &sp, (int)B, items.data(), rs.data());
    for (size_t b = 0; b < B; b++) { const size_t n = fs[b].px.size(); vpriors3d[b].resize(n); vhasprior3d[b].resize(n); vskip[b].resize(n); }
    return rc;
}

}  // namespace ov2
