// kfreq_run.cpp -- test driver for the frame-versus-keyframe passes through the C++ adapter (ov2slam_amd/host/visual_front_end.hpp):
// reads the case file written by tests/test_gpu_kfreq.py (the keyframe side in no particular order), runs ov2::computeParallax in the
// five forms the reference calls, ov2::checkNewKfReq and ov2::epipolarFilter2d on every scene, one call each and then as batches, and
// writes per scene: 5 parallaxes, {decision, reason, noccupcells, nb3dkps}, the bad keypoint ids and the errors.  File format (both
// ways): a sequence of arrays, each an int64 byte count followed by the raw bytes.
#include <cstdio>
#include "../../ov2slam_amd/host/visual_front_end.hpp"

template <class T> static std::vector<T> rd(FILE *f)
{
    long long nb = 0;
    if (fread(&nb, 8, 1, f) != 1) throw std::runtime_error("short case file");
    std::vector<T> v((size_t)nb / sizeof(T));
    if (nb && fread(v.data(), 1, (size_t)nb, f) != (size_t)nb) throw std::runtime_error("short case file");
    return v;
}
template <class T> static void wr(FILE *f, const T *p, size_t n)
{
    const long long nb = (long long)(n * sizeof(T));
    fwrite(&nb, 8, 1, f);
    if (nb) fwrite(p, 1, (size_t)nb, f);
}
static std::vector<ov2::Point2f> pts(const std::vector<float> &v)
{
    std::vector<ov2::Point2f> p(v.size() / 2);
    for (size_t i = 0; i < p.size(); i++) p[i] = ov2::Point2f(v[2 * i], v[2 * i + 1]);
    return p;
}
static void need(int rc, const char *what)
{
    if (rc != OV2_OK) throw std::runtime_error(std::string(what) + ": " + ov2_last_error());
}
struct Form { bool unrot; int filter, stat; };
static const Form FORMS[5] = {{true, OV2_FKF_ALL, OV2_FKF_MEDIAN}, {false, OV2_FKF_ALL, OV2_FKF_AVG}, {false, OV2_FKF_ONLY_2D, OV2_FKF_AVG},
                              {true, OV2_FKF_ALL, OV2_FKF_AVG_WIDE}, {true, OV2_FKF_ONLY_3D, OV2_FKF_AVG_WIDE}};
static void dump(FILE *f, const float par[5], const ov2_kf_decision_result &d, const std::vector<int> &bad, const std::vector<float> &err)
{
    wr(f, par, 5);
    const int v[4] = {d.decision, d.reason, d.noccupcells, d.nb3dkps};
    wr(f, v, 4);
    wr(f, bad.data(), bad.size());
    wr(f, err.data(), err.size());
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: kfreq_run <case> <result>\n"); return 2; }
    try {
        FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
        if (!fi || !fo) throw std::runtime_error("cannot open files");
        const std::vector<double> K = rd<double>(fi);
        const std::vector<int> g = rd<int>(fi);                    // ncellsize, nbwcells, nbhcells, nbmaxkps, stereo, scenes
        const std::vector<float> e = rd<float>(fi);                // finit_parallax, fransac_err
        ov2::KfReqParams P;
        for (int j = 0; j < 4; j++) P.K[j] = K[j];
        P.ncellsize = g[0]; P.nbwcells = g[1]; P.nbhcells = g[2]; P.nbmaxkps = g[3]; P.stereo = g[4] != 0; P.finit_parallax = e[0];
        std::vector<ov2::FrameVsKeyframe> fs((size_t)g[5]);
        std::vector<double> vF;
        for (ov2::FrameVsKeyframe &f : fs) {
            f.cur_lmid = rd<int>(fi); f.cur_px = pts(rd<float>(fi)); f.cur_unpx = pts(rd<float>(fi)); f.cur_bv = rd<double>(fi);
            f.cur_is3d = rd<uint8_t>(fi);
            const std::vector<double> twc = rd<double>(fi);
            f.kf_lmid = rd<int>(fi); f.kf_unpx = pts(rd<float>(fi));
            const std::vector<double> tcw = rd<double>(fi);
            for (int j = 0; j < 7; j++) { f.cur_Twc[j] = twc[j]; f.kf_Tcw[j] = tcw[j]; }
            const std::vector<int> s = rd<int>(fi);                // cur_id, kf_id, kf_nb3dkps, localba_is_on, noccupcells, nb3dkps
            f.cur_id = s[0]; f.kf_id = s[1]; f.kf_nb3dkps = s[2]; f.localba_is_on = s[3] != 0; f.noccupcells = s[4]; f.nb3dkps = s[5];
            const std::vector<double> t = rd<double>(fi);
            f.cur_time = t[0]; f.kf_time = t[1];
            const std::vector<double> F = rd<double>(fi);
            vF.insert(vF.end(), F.begin(), F.end());
        }
        ov2::Context ctx(0);
        for (size_t b = 0; b < fs.size(); b++) {                   // one call per scene
            float par[5];
            for (int k = 0; k < 5; k++) {
                ov2_parallax_result r{};
                need(ov2::computeParallax(ctx, P, fs[b], FORMS[k].unrot, FORMS[k].filter, FORMS[k].stat, r), "computeParallax");
                par[k] = r.parallax;
            }
            ov2_kf_decision_result d{};
            need(ov2::checkNewKfReq(ctx, P, fs[b], d), "checkNewKfReq");
            std::vector<int> bad;
            std::vector<float> err;
            need(ov2::epipolarFilter2d(ctx, fs[b], &vF[9 * b], e[1], bad, &err), "epipolarFilter2d");
            dump(fo, par, d, bad, err);
        }
        std::vector<ov2_parallax_result> pr[5];
        for (int k = 0; k < 5; k++) need(ov2::computeParallax(ctx, P, fs, FORMS[k].unrot, FORMS[k].filter, FORMS[k].stat, pr[k]), "computeParallax (batch)");
        std::vector<ov2_kf_decision_result> ds;
        need(ov2::checkNewKfReq(ctx, P, fs, ds), "checkNewKfReq (batch)");
        std::vector<std::vector<int>> bads;
        std::vector<std::vector<float>> errs;
        need(ov2::epipolarFilter2d(ctx, fs, vF, e[1], bads, &errs), "epipolarFilter2d (batch)");
        for (size_t b = 0; b < fs.size(); b++) {
            const float par[5] = {pr[0][b].parallax, pr[1][b].parallax, pr[2][b].parallax, pr[3][b].parallax, pr[4][b].parallax};
            dump(fo, par, ds[b], bads[b], errs[b]);
        }
        fclose(fi); fclose(fo);
    } catch (const std::exception &ex) {
        fprintf(stderr, "%s\n", ex.what());
        return 1;
    }
    return 0;
}
