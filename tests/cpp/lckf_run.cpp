// lckf_run.cpp -- test driver for the loop closer's keyframe preparation through the C++ adapter (ov2slam_amd/host/loop_closer.hpp):
// reads the case file written by tests/test_gpu_lckf.py (width, height, retain, the image, the exclusion points), runs
// ov2::LoopCloser::detectAdditionalKeypoints in both orders and writes, per order, the pixels, the responses and the descriptors.
// File format (both ways): a sequence of arrays, each an int64 byte count followed by the raw bytes.
#include <cstdio>
#include "../../ov2slam_amd/host/loop_closer.hpp"

template <class T> static std::vector<T> rd(FILE *f)
{
    long long nb = 0;
    if (fread(&nb, 8, 1, f) != 1) throw std::runtime_error("short case file");
    std::vector<T> v((size_t)nb / sizeof(T));
    if (nb && fread(v.data(), 1, (size_t)nb, f) != (size_t)nb) throw std::runtime_error("short case file");
    return v;
}
template <class T> static void wr(FILE *f, const std::vector<T> &v)
{
    const long long nb = (long long)(v.size() * sizeof(T));
    fwrite(&nb, 8, 1, f);
    if (nb) fwrite(v.data(), 1, (size_t)nb, f);
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: lckf_run <case> <result>\n"); return 2; }
    try {
        FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
        if (!fi || !fo) throw std::runtime_error("cannot open files");
        const std::vector<int> dims = rd<int>(fi);                   // w, h, threshold, retain, radius
        const std::vector<uint8_t> img = rd<uint8_t>(fi);
        const std::vector<float> ex = rd<float>(fi);
        if (dims.size() != 5 || img.size() != (size_t)dims[0] * (size_t)dims[1]) throw std::runtime_error("bad case file");
        std::vector<ov2::Point2f> excl;
        for (size_t i = 0; i + 1 < ex.size(); i += 2) excl.emplace_back(ex[i], ex[i + 1]);
        ov2::Context ctx(0);
        ov2::LoopCloser lc;
        lc.setKeyframePreparation(dims[2], dims[3], dims[4]);
        const ov2::Image8 im(img.data(), dims[0], dims[1], dims[0]);
        for (const auto order : {ov2::LoopCloser::Order::Raster, ov2::LoopCloser::Order::Reference}) {
            std::vector<ov2::Point2f> px{{-1.f, -1.f}};              // whatever was there is replaced
            std::vector<float> resp;
            std::vector<uint8_t> desc;
            const int rc = lc.detectAdditionalKeypoints(ctx, im, excl, px, resp, desc, order);
            if (rc != OV2_OK) throw std::runtime_error(std::string("detectAdditionalKeypoints: ") + ov2_last_error());
            if (resp.size() != px.size() || desc.size() != 32 * px.size()) throw std::runtime_error("outputs of different lengths");
            std::vector<float> flat;
            for (const auto &p : px) { flat.push_back(p.x); flat.push_back(p.y); }
            wr(fo, flat); wr(fo, resp); wr(fo, desc);
        }
        std::vector<ov2::Point2f> px;
        std::vector<float> resp;
        std::vector<uint8_t> desc;
        if (lc.detectAdditionalKeypoints(ctx, ov2::Image8(), excl, px, resp, desc) != OV2_EINVAL) throw std::runtime_error("an empty image did not fail");
        fclose(fi); fclose(fo);
    } catch (const std::exception &ex) {
        fprintf(stderr, "%s\n", ex.what());
        return 1;
    }
    return 0;
}
