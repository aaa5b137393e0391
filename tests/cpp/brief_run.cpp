// brief_run.cpp -- test driver for FeatureExtractor::describeBRIEF of ov2slam_amd/host/feature_extractor.hpp: runs the host-image
// form and the FrameTracker form (raw current frame, CLAHE on) on the case file written by tests/test_gpu_brief.py and dumps what
// they return, next to what the C ABI returns for the same points.  File format (both ways): a sequence of arrays, each an int64
// byte count followed by the raw bytes.
#include <cstdio>
#include "../../ov2slam_amd/host/feature_extractor.hpp"
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
static void wr_desc(FILE *f, const std::vector<ov2::FeatureExtractor::BriefDescriptor> &v) { wr(f, v.empty() ? nullptr : v[0].data(), 32 * v.size()); }

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: brief_run <case> <result>\n"); return 2; }
    try {
        FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
        if (!fi || !fo) throw std::runtime_error("cannot open files");
        const std::vector<int> dims = rd<int>(fi);                       // w, h
        const int w = dims[0], h = dims[1];
        const std::vector<uint8_t> img = rd<uint8_t>(fi);
        const std::vector<float> xy = rd<float>(fi);
        std::vector<ov2::Point2f> pts(xy.size() / 2);
        for (size_t i = 0; i < pts.size(); i++) pts[i] = ov2::Point2f(xy[2 * i], xy[2 * i + 1]);
        ov2::Context ctx(0);
        const ov2::Image8 I(img.data(), w, h, w);
        ov2::FeatureExtractor fx(0, 0, 0.001, 10);
        std::vector<uint8_t> valid;

        const auto d_host = fx.describeBRIEF(ctx, I, pts, valid);
        if (d_host.size() != pts.size()) throw std::runtime_error(std::string("describeBRIEF (host image) failed: ") + ov2_last_error());
        wr_desc(fo, d_host); wr(fo, valid.data(), valid.size());

        ov2::FrameTracker ft(ctx, w, h, 9, 3, 30, 0.01f, 30.f, 0.5f, true, 3.0, 512);
        std::vector<ov2::Point2f> none, nonep;
        std::vector<bool> st;
        bool p3p = false;
        if (!ft.trackFrame(I, none, nonep, std::vector<uint8_t>(), true, st, p3p)) throw std::runtime_error("trackFrame failed");
        const auto d_trk = fx.describeBRIEF(ft.get(), pts, valid);
        if (d_trk.size() != pts.size()) throw std::runtime_error(std::string("describeBRIEF (tracker) failed: ") + ov2_last_error());
        wr_desc(fo, d_trk); wr(fo, valid.data(), valid.size());

        std::vector<uint8_t> d_abi(32 * pts.size()), v_abi(pts.size());
        if (ov2_describe_brief(ctx.get(), img.data(), w, h, w, xy.data(), (int)pts.size(), d_abi.data(), v_abi.data()) != OV2_OK)
            throw std::runtime_error(std::string("ov2_describe_brief: ") + ov2_last_error());
        wr(fo, d_abi.data(), d_abi.size()); wr(fo, v_abi.data(), v_abi.size());

        const std::vector<ov2::Point2f> empty;
        const auto d_empty = fx.describeBRIEF(ctx, I, empty, valid);
        const int n_empty = (int)d_empty.size();
        wr(fo, &n_empty, 1);
        fclose(fi); fclose(fo);
    } catch (const std::exception &e) {
        fprintf(stderr, "brief_run: %s\n", e.what());
        return 1;
    }
    return 0;
}
