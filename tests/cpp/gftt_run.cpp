// gftt_run.cpp -- test driver for detectGFTT through the C++ adapter (ov2slam_amd/host/feature_extractor.hpp: host image and
// device pyramid forms) and through the reference's own signature (ov2slam_amd/host/verbatim.hpp, built with -DOV2_WITH_OPENCV
// against tests/fake_opencv), on the case file written by tests/test_gpu_gftt.py; dumps what each form returns, next to what the
// C ABI returns for the same inputs.  File format (both ways): a sequence of arrays, each an int64 byte count followed by the raw bytes.
#include <cstdio>
#include "../../ov2slam_amd/host/verbatim.hpp"

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
static void wr_pts(FILE *f, const std::vector<cv::Point2f> &v) { wr(f, v.empty() ? nullptr : &v[0].x, 2 * v.size()); }

static cv::Mat mat(std::vector<uint8_t> &buf, int w, int h, int step)
{
    cv::Mat m;
    m.data = buf.empty() ? nullptr : buf.data(); m.cols = w; m.rows = h; m.step.v = (size_t)step;
    return m;
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: gftt_run <case> <result>\n"); return 2; }
    try {
        FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
        if (!fi || !fo) throw std::runtime_error("cannot open files");
        const std::vector<int> a = rd<int>(fi);                          // w, h, stride, nmaxpts, nmaxdist, nbmax
        const std::vector<double> q = rd<double>(fi);                    // dmaxquality
        std::vector<uint8_t> img = rd<uint8_t>(fi);                      // h rows of `stride` bytes
        std::vector<uint8_t> roi = rd<uint8_t>(fi);                      // empty, or h rows of `stride` bytes
        const std::vector<float> xy = rd<float>(fi);
        const int w = a[0], h = a[1], stride = a[2], nbmax = a[5];
        std::vector<cv::Point2f> cur(xy.size() / 2);
        for (size_t i = 0; i < cur.size(); i++) cur[i] = cv::Point2f(xy[2 * i], xy[2 * i + 1]);
        ov2::Context ctx(0);
        ov2::FeatureExtractor fx((size_t)a[3], (size_t)a[4], q[0], 10);
        const ov2::Image8 I(img.data(), w, h, stride);
        const ov2::Image8 R = roi.empty() ? ov2::Image8() : ov2::Image8(roi.data(), w, h, stride);

        const std::vector<cv::Point2f> p_host = fx.detectGFTT(ctx, I, cur, R, nbmax);
        wr_pts(fo, p_host);

        ov2::Pyramid pyr;
        if (pyr.build(ctx, I, 9, 3) != OV2_OK) throw std::runtime_error(std::string("pyramid: ") + ov2_last_error());
        const std::vector<cv::Point2f> p_pyr = fx.detectGFTT(ctx, pyr.get(), cur, R, nbmax);
        wr_pts(fo, p_pyr);

        ov2::verbatim::FeatureExtractor vx((size_t)a[3], (size_t)a[4], q[0], 10);
        const cv::Mat im = mat(img, w, h, stride), rm = mat(roi, w, h, stride);
        const std::vector<cv::Point2f> p_verb = vx.detectGFTT(im, cur, rm, nbmax);
        wr_pts(fo, p_verb);
        const int derived[2] = {(int)vx.nmindist(), vx.dminquality() == q[0] / 2. ? 1 : 0};
        wr(fo, derived, 2);

        std::vector<float> o_abi(2 * (size_t)(nbmax != -1 ? nbmax : a[3]) + 2);
        ov2_gftt_params gp;
        ov2_gftt_params_init(a[3], a[4], q[0], &gp);
        int n = -1;
        if (ov2_detect_gftt(ctx.get(), img.data(), w, h, stride, roi.empty() ? nullptr : roi.data(), stride, &gp, xy.empty() ? nullptr : xy.data(),
                            (int)cur.size(), nbmax, 1, o_abi.data(), (int)(o_abi.size() / 2), &n) != OV2_OK)
            throw std::runtime_error(std::string("ov2_detect_gftt: ") + ov2_last_error());
        wr(fo, o_abi.data(), 2 * (size_t)n);

        // the reference's default constructor (nmaxpts_ 0 here: the early return) and an invalid nbmax: empty lists, no exception
        ov2::verbatim::FeatureExtractor vdef;
        const int n_edge[2] = {(int)vdef.detectGFTT(im, cur, rm).size(), (int)fx.detectGFTT(ctx, I, cur, R, 0).size()};
        wr(fo, n_edge, 2);
        fclose(fi); fclose(fo);
    } catch (const std::exception &e) {
        fprintf(stderr, "gftt_run: %s\n", e.what());
        return 1;
    }
    return 0;
}
