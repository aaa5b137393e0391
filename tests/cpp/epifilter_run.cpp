// epifilter_run.cpp -- test driver for ov2::epipolar2d2dFiltering (ov2slam_amd/host/visual_front_end.hpp): reads the text case file
// written by tests/test_gpu_epifilter.py (the keyframe side in no particular order), runs the adapter once alone and once as a batch
// of two, and prints "action m n_removed_ransac n_removed_sampson" and, on a second line, the lmids to remove in the reference's
// order.  Case file: K (4) stereo mono nransac_iter threshold probability fransac_err n_rows / n_cur n_kf nbkfs seed nb3dkps / cur_Twc /
// kf_Tcw / kf_Twc / per current keypoint: lmid is3d px (2) unpx (2) bv (3) / per keyframe keypoint: lmid unpx (2) bv (3).
#include <cstdio>
#include <fstream>
#include "../../ov2slam_amd/host/visual_front_end.hpp"

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: epifilter_run <case>\n"); return 2; }
    try {
        std::ifstream fi(argv[1]);
        if (!fi) throw std::runtime_error("cannot open the case file");
        ov2::EpipolarFilterParams P;
        ov2::EpipolarFilterInput in;
        int stereo = 0, mono = 0, n_cur = 0, n_kf = 0;
        fi >> P.kf.K[0] >> P.kf.K[1] >> P.kf.K[2] >> P.kf.K[3] >> stereo >> mono >> P.nransac_iter >> P.threshold >> P.probability >>
            P.fransac_err >> P.n_rows;
        P.kf.stereo = stereo != 0; P.mono = mono != 0;
        fi >> n_cur >> n_kf >> in.nbkfs >> in.seed >> in.f.nb3dkps;
        for (double &v : in.f.cur_Twc) fi >> v;
        for (double &v : in.f.kf_Tcw) fi >> v;
        for (double &v : in.kf_Twc) fi >> v;
        for (int i = 0; i < n_cur; i++) {
            int lmid = 0, is3d = 0;
            float px[4];
            double bv[3];
            fi >> lmid >> is3d >> px[0] >> px[1] >> px[2] >> px[3] >> bv[0] >> bv[1] >> bv[2];
            in.f.cur_lmid.push_back(lmid); in.f.cur_is3d.push_back((uint8_t)is3d);
            in.f.cur_px.push_back(ov2::Point2f(px[0], px[1])); in.f.cur_unpx.push_back(ov2::Point2f(px[2], px[3]));
            in.f.cur_bv.insert(in.f.cur_bv.end(), bv, bv + 3);
        }
        for (int j = 0; j < n_kf; j++) {
            int lmid = 0;
            float un[2];
            double bv[3];
            fi >> lmid >> un[0] >> un[1] >> bv[0] >> bv[1] >> bv[2];
            in.f.kf_lmid.push_back(lmid); in.f.kf_unpx.push_back(ov2::Point2f(un[0], un[1]));
            in.kf_bv.insert(in.kf_bv.end(), bv, bv + 3);
        }
        if (!fi) throw std::runtime_error("short case file");
        ov2::Context ctx(0);
        ov2::EpipolarFilterOutput one;
        int rc = ov2::epipolar2d2dFiltering(ctx, P, in, one);
        if (rc != OV2_OK) throw std::runtime_error(std::string("epipolar2d2dFiltering: ") + ov2_last_error());
        std::vector<ov2::EpipolarFilterOutput> two;
        rc = ov2::epipolar2d2dFiltering(ctx, P, std::vector<ov2::EpipolarFilterInput>(2, in), two);
        if (rc != OV2_OK) throw std::runtime_error(std::string("epipolar2d2dFiltering (batch): ") + ov2_last_error());
        for (const ov2::EpipolarFilterOutput &o : two)
            if (o.vremove != one.vremove || o.r.action != one.r.action || o.removed != one.removed)
                throw std::runtime_error("the batch form differs from the single call");
        printf("%d %d %d %d\n", one.r.action, one.r.m, one.r.n_removed_ransac, one.r.n_removed_sampson);
        for (int v : one.vremove) printf("%d ", v);
        printf("\n");
    } catch (const std::exception &e) {
        fprintf(stderr, "epifilter_run: %s\n", e.what());
        return 1;
    }
    return 0;
}
