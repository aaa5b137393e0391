// compile_check.cpp -- keeps the C++ adapters compiling (g++ -fsyntax-only, see tests/test_abi.py)
#include "feature_tracker.hpp"
#include "feature_extractor.hpp"
#include "optimizer.hpp"
#include "camera_calibration.hpp"
#include "visual_front_end.hpp"
#include "slam_gpu.hpp"
#include "mapper.hpp"
#include "multi_view_geometry.hpp"
#include "loop_closer.hpp"
// the adapters that are free functions: taking their addresses keeps their signatures checked
static auto *const check_ceres_pnp = &ov2::ceresPnP;
static auto *const check_ceres_pnp_fused = &ov2::ceresPnPFused;
static int (*const check_compute_pose)(ov2::Context &, const ov2::ComputePoseParams &, const ov2::ComputePoseInput &, ov2::ComputePoseOutput &) = &ov2::computePose;
static auto *const check_p3p_ransac = &ov2::p3pRansac;
static auto *const check_5pt = &ov2::compute5ptEssentialMatrix;
// the rectification adapters (CameraCalibration, FrameTracker), by address too
static auto const check_undist_maps = &ov2::CameraCalibration::setUndistMaps;
static auto const check_rectify = &ov2::CameraCalibration::rectifyImage;
static auto const check_rect_map = &ov2::CameraCalibration::rectMap;
static auto const check_set_rect = &ov2::FrameTracker::setRectification;
// the loop closer's descriptor matching, both overloads
static int (ov2::LoopCloser::*const check_knn)(ov2::Context &, const std::vector<uint8_t> &, const std::vector<int> &, const std::vector<uint8_t> &,
                                               const std::vector<int> &, std::vector<std::pair<int, int>> &) const = &ov2::LoopCloser::knnMatching;
static int (ov2::LoopCloser::*const check_knn_batch)(ov2::Context &, const std::vector<ov2::KnnMatchingInput> &,
                                                     std::vector<std::vector<std::pair<int, int>>> &) const = &ov2::LoopCloser::knnMatching;
// the keyframe preparation, host image and tracker forms, and the host-side order helper
static int (ov2::LoopCloser::*const check_lckf)(ov2::Context &, const ov2::Image8 &, const std::vector<ov2::Point2f> &, std::vector<ov2::Point2f> &,
                                                std::vector<float> &, std::vector<uint8_t> &, ov2::LoopCloser::Order) const = &ov2::LoopCloser::detectAdditionalKeypoints;
static int (ov2::LoopCloser::*const check_lckf_trk)(ov2_tracker *, const std::vector<ov2::Point2f> &, std::vector<ov2::Point2f> &,
                                                    std::vector<float> &, std::vector<uint8_t> &, ov2::LoopCloser::Order) const = &ov2::LoopCloser::detectAdditionalKeypoints;
static auto *const check_retain_order = &ov2::retainBestReferenceOrder;
// the loop local-map tracking, both overloads, its settings and the host-side walk
static int (ov2::LoopCloser::*const check_loopmap)(ov2::Context &, const ov2::LoopMapInput &, std::vector<std::pair<int, int>> &,
                                                   ov2::LoopMapOutput *) const = &ov2::LoopCloser::trackLoopLocalMap;
static int (ov2::LoopCloser::*const check_loopmap_batch)(ov2::Context &, const std::vector<ov2::LoopMapInput> &,
                                                         std::vector<std::vector<std::pair<int, int>>> &,
                                                         std::vector<ov2::LoopMapOutput> *) const = &ov2::LoopCloser::trackLoopLocalMap;
static auto const check_set_loopmap = &ov2::LoopCloser::setLoopMapMatching;
static auto *const check_loopmap_order = &ov2::loopLocalMapReferenceOrder;
// frame versus previous keyframe: computeParallax / checkNewKfReq / epipolarFilter2d, single and batch
static int (*const check_parallax)(ov2::Context &, const ov2::KfReqParams &, const ov2::FrameVsKeyframe &, bool, int, int, ov2_parallax_result &) = &ov2::computeParallax;
static int (*const check_parallax_batch)(ov2::Context &, const ov2::KfReqParams &, const std::vector<ov2::FrameVsKeyframe> &, bool, int, int,
                                         std::vector<ov2_parallax_result> &) = &ov2::computeParallax;
static int (*const check_kfreq)(ov2::Context &, const ov2::KfReqParams &, const ov2::FrameVsKeyframe &, ov2_kf_decision_result &) = &ov2::checkNewKfReq;
static int (*const check_kfreq_batch)(ov2::Context &, const ov2::KfReqParams &, const std::vector<ov2::FrameVsKeyframe> &,
                                      std::vector<ov2_kf_decision_result> &) = &ov2::checkNewKfReq;
static int (*const check_epi2d)(ov2::Context &, const ov2::FrameVsKeyframe &, const double *, float, std::vector<int> &, std::vector<float> *) = &ov2::epipolarFilter2d;
static int (*const check_epi2d_batch)(ov2::Context &, const std::vector<ov2::FrameVsKeyframe> &, const std::vector<double> &, float,
                                      std::vector<std::vector<int>> &, std::vector<std::vector<float>> *) = &ov2::epipolarFilter2d;
static auto const check_kf_sort = &ov2::detail::sortKeyframeByLmid;
// epipolar2d2dFiltering as one device chain, single and batch
static int (*const check_epif)(ov2::Context &, const ov2::EpipolarFilterParams &, const ov2::EpipolarFilterInput &, ov2::EpipolarFilterOutput &) = &ov2::epipolar2d2dFiltering;
static int (*const check_epif_batch)(ov2::Context &, const ov2::EpipolarFilterParams &, const std::vector<ov2::EpipolarFilterInput> &,
                                     std::vector<ov2::EpipolarFilterOutput> &) = &ov2::epipolar2d2dFiltering;
// trackMono's un-initialised branch (checkReadyForInit) as one device chain, single and batch
static int (*const check_minit)(ov2::Context &, const ov2::MonoInitParams &, const ov2::MonoInitInput &, ov2::MonoInitOutput &) = &ov2::checkReadyForInit;
static int (*const check_minit_batch)(ov2::Context &, const ov2::MonoInitParams &, const std::vector<ov2::MonoInitInput> &,
                                      std::vector<ov2::MonoInitOutput> &) = &ov2::checkReadyForInit;
// the tracking priors: kltPriors / stereoPriors, single and batch, and their host-only helpers
static int (*const check_klt_priors)(ov2::Context &, const ov2::ProjectionCamera &, bool, const ov2::KltPriorsInput &, std::vector<ov2::Point2f> &,
                                     std::vector<uint8_t> &) = &ov2::kltPriors;
static int (*const check_klt_priors_batch)(ov2::Context &, const ov2::ProjectionCamera &, bool, const std::vector<ov2::KltPriorsInput> &,
                                           std::vector<std::vector<ov2::Point2f>> &, std::vector<std::vector<uint8_t>> &) = &ov2::kltPriors;
static int (*const check_stereo_priors)(ov2::Context &, const ov2::StereoPriorsParams &, const ov2::StereoPriorsInput &, std::vector<ov2::Point2f> &,
                                        std::vector<uint8_t> &, std::vector<uint8_t> &) = &ov2::stereoPriors;
static int (*const check_stereo_priors_batch)(ov2::Context &, const ov2::StereoPriorsParams &, const std::vector<ov2::StereoPriorsInput> &,
                                              std::vector<std::vector<ov2::Point2f>> &, std::vector<std::vector<uint8_t>> &,
                                              std::vector<std::vector<uint8_t>> &) = &ov2::stereoPriors;
static auto const check_cell_table = &ov2::detail::buildCellTable;
static auto const check_pack_klt = &ov2::detail::packKltPriors;
// the motion model: the reference's three methods
static int (ov2::MotionModel::*const check_motion_apply)(ov2::Context &, double *, double, double *, bool *) = &ov2::MotionModel::applyMotionModel;
static int (ov2::MotionModel::*const check_motion_update)(ov2::Context &, const double *, double) = &ov2::MotionModel::updateMotionModel;
static void (ov2::MotionModel::*const check_motion_reset)() = &ov2::MotionModel::reset;

int main() { return check_motion_apply && check_motion_update && check_motion_reset && check_klt_priors && check_klt_priors_batch && check_stereo_priors && check_stereo_priors_batch && check_cell_table && check_pack_klt && check_parallax && check_parallax_batch && check_kfreq && check_kfreq_batch && check_epi2d && check_epi2d_batch && check_kf_sort && check_loopmap && check_loopmap_batch && check_set_loopmap && check_loopmap_order && check_lckf && check_lckf_trk && check_retain_order && check_knn && check_knn_batch && check_ceres_pnp && check_p3p_ransac && check_5pt && check_undist_maps && check_rectify && check_rect_map && check_set_rect ? 0 : 1; }
