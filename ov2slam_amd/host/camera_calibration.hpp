// camera_calibration.hpp -- host-side adapter mirroring the reference's per-keypoint
// CameraCalibration::undistortImagePoint (/root/reference/src/camera_calibration.cpp:313-333) and
// Frame::computeKeypoint (src/frame.cpp:246-254) on top of ov2_compute_keypoints (one launch for a
// whole vector of keypoints instead of one cv::undistortPoints call per point), and CameraCalibration::rectifyImage
// (src/camera_calibration.cpp:233-241: cv::remap through undist_map_x_ / undist_map_y_) on top of ov2_rectify_h.
#pragma once
#include <vector>
#include <array>
#include <memory>
#include "ov2_types.hpp"

namespace ov2 {

struct CameraCalibration {
    enum Model { Pinhole = OV2_CAM_PINHOLE, Fisheye = OV2_CAM_FISHEYE };
    Model model_ = Pinhole;
    double K_[4] = {1., 1., 0., 0.};          // fx, fy, cx, cy
    std::vector<double> D_;                   // empty after rectification (Dcv_.release(), camera_calibration.cpp:107)
    double iK_[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};   // row-major K_.inverse(), filled by the caller from its Eigen matrix

    // Frame::computeKeypoint for a vector of raw pixel positions: unpx_ and bv_ of every keypoint
    int computeKeypoints(ov2_ctx *ctx, const std::vector<Point2f> &vpx, std::vector<Point2f> &vunpx,
                         std::vector<std::array<double, 3>> *vbv = nullptr) const
    {
        vunpx.resize(vpx.size());
        if (vbv) vbv->resize(vpx.size());
        if (vpx.empty()) return OV2_OK;
        return ov2_compute_keypoints(ctx, (int)model_, K_, D_.empty() ? nullptr : D_.data(), (int)D_.size(), iK_,
                                     &vpx[0].x, (int)vpx.size(), &vunpx[0].x, vbv ? (*vbv)[0].data() : nullptr);
    }

    // undist_map_x_ / undist_map_y_ as setUndistMap (form OV2_MAP_F32: map1 = x, map2 = y, w * h floats each,
    // camera_calibration.cpp:92 / :97) or setUndistStereoMap (form OV2_MAP_FIXED: map1 = w * h int16 pairs, map2 = w * h uint16,
    // :141 / :145) leave them: the caller computes them once at start-up (cv::initUndistortRectifyMap) and hands the Mats' data
    // over.  The arrays are copied; the device map is created by the first rectifyImage / rectMap call.  As in the reference the
    // calibration is the rectified one from then on: D_ is emptied (Dcv_.release(), :107 / :161).
    void setUndistMaps(int form, const void *map1, const void *map2, int w, int h)
    {
        const size_t n = (size_t)w * (size_t)h, b1 = 4 * n, b2 = form == OV2_MAP_F32 ? 4 * n : 2 * n;     // bytes of map1 / map2
        map_form_ = form; map_w_ = w; map_h_ = h;
        map1_.assign((const uint8_t *)map1, (const uint8_t *)map1 + b1);
        map2_.assign((const uint8_t *)map2, (const uint8_t *)map2 + b2);
        rect_map_.reset();
        D_.clear();
    }

    // the device map (ov2_rectmap) of the maps above, created on first use: what FrameTracker::setRectification and
    // ov2_pyr_build_rect_h take.  nullptr when no maps are set or they violate the contract (ov2_last_error says why).
    // It lives as long as the last copy of this calibration: keep one while a tracker uses the map.
    const ov2_rectmap *rectMap(ov2_ctx *ctx)
    {
        if (!rect_map_ && !map1_.empty()) {
            ov2_rectmap *m = nullptr;
            if (ov2_rectmap_create(ctx, map_w_, map_h_, map_form_, map1_.data(), map2_.data(), &m) != OV2_OK) return nullptr;
            rect_map_ = std::shared_ptr<ov2_rectmap>(m, ov2_rectmap_destroy);
        }
        return rect_map_.get();
    }

    // CameraCalibration::rectifyImage(img, rect): cv::remap(img, rect, undist_map_x_, undist_map_y_, cv::INTER_LINEAR) when the
    // maps are set; without maps the reference's `rect = img` shares the buffer (:240), so rect must be img and nothing is done.
    // img / rect: h rows of w bytes (the maps' size), `stride` / `rect_stride` bytes apart; rect == img is allowed (the reference
    // rectifies in place, src/ov2slam.cpp:242).
    int rectifyImage(ov2_ctx *ctx, const uint8_t *img, int stride, uint8_t *rect, int rect_stride)
    {
        if (map1_.empty()) return img && rect == img ? OV2_OK : OV2_EINVAL;
        const ov2_rectmap *m = rectMap(ctx);
        return m ? ov2_rectify_h(ctx, m, img, stride, rect, rect_stride) : OV2_EINVAL;
    }

    // single-point form with the reference's signature
    Point2f undistortImagePoint(ov2_ctx *ctx, const Point2f &pt) const
    {
        std::vector<Point2f> in{pt}, out;
        return computeKeypoints(ctx, in, out) == OV2_OK ? out[0] : pt;
    }

    int map_form_ = OV2_MAP_F32, map_w_ = 0, map_h_ = 0;
    std::vector<uint8_t> map1_, map2_;
    std::shared_ptr<ov2_rectmap> rect_map_;
};

} // namespace ov2
