// rectify_run.cpp -- test driver for the rectification adapters of ov2slam_amd/host: CameraCalibration::setUndistMaps / rectifyImage
// (out of place and in place, strided buffers) and FrameTracker::setRectification on the case file written by
// tests/test_gpu_rectify.py; dumps what they return.  File format (both ways): a sequence of arrays, each an int64 byte count
// followed by the raw bytes.
#include <cstdio>
#include "../../ov2slam_amd/host/camera_calibration.hpp"
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

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: rectify_run <case> <result>\n"); return 2; }
    try {
        FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
        if (!fi || !fo) throw std::runtime_error("cannot open files");
        const std::vector<int> dims = rd<int>(fi);                       // w, h, form, src stride, dst stride
        const int w = dims[0], h = dims[1], form = dims[2], sstride = dims[3], dstride = dims[4];
        const std::vector<uint8_t> map1 = rd<uint8_t>(fi), map2 = rd<uint8_t>(fi);
        const std::vector<uint8_t> img = rd<uint8_t>(fi);                // h rows, sstride apart
        ov2::Context ctx(0);
        ov2::CameraCalibration cal;
        cal.D_ = {-0.28, 0.07, 2e-4, 2e-5};
        // no maps yet: rectifyImage is the reference's `rect = img`
        std::vector<uint8_t> same(img);
        if (cal.rectifyImage(ctx.get(), same.data(), sstride, same.data(), sstride) != OV2_OK || same != img) throw std::runtime_error("rectifyImage without maps");
        cal.setUndistMaps(form, map1.data(), map2.data(), w, h);
        if (!cal.D_.empty()) throw std::runtime_error("setUndistMaps keeps D_");

        std::vector<uint8_t> rect((size_t)h * dstride, 0xA5);            // the padding must keep its canary
        if (cal.rectifyImage(ctx.get(), img.data(), sstride, rect.data(), dstride) != OV2_OK)
            throw std::runtime_error(std::string("rectifyImage: ") + ov2_last_error());
        wr(fo, rect.data(), rect.size());

        std::vector<uint8_t> inplace(img);                               // rect == img
        if (cal.rectifyImage(ctx.get(), inplace.data(), sstride, inplace.data(), sstride) != OV2_OK)
            throw std::runtime_error(std::string("rectifyImage in place: ") + ov2_last_error());
        wr(fo, inplace.data(), inplace.size());

        // FrameTracker fed the raw frame (no CLAHE: level 0 of its pyramid is the rectified frame itself)
        ov2::FrameTracker ft(ctx, w, h, 9, 3, 30, 0.01f, 30.f, 0.5f, false, 3.0, 64);
        if (!ft.setRectification(cal.rectMap(ctx.get()))) throw std::runtime_error(std::string("setRectification: ") + ov2_last_error());
        std::vector<ov2::Point2f> none, nonep;
        std::vector<bool> st;
        bool p3p = false;
        if (!ft.trackFrame(ov2::Image8(img.data(), w, h, sstride), none, nonep, std::vector<uint8_t>(), true, st, p3p)) throw std::runtime_error("trackFrame failed");
        std::vector<uint8_t> l0((size_t)w * h);
        if (ov2_pyr_download(ctx.get(), ft.curPyr(), 0, 0, l0.data(), nullptr) != OV2_OK) throw std::runtime_error(std::string("ov2_pyr_download: ") + ov2_last_error());
        wr(fo, l0.data(), l0.size());
        if (!ft.setRectification(nullptr)) throw std::runtime_error("setRectification(nullptr)");
        fclose(fi); fclose(fo);
    } catch (const std::exception &e) {
        fprintf(stderr, "rectify_run: %s\n", e.what());
        return 1;
    }
    return 0;
}
