// p3p_run.cpp -- test driver for the absolute-pose search through the C++ adapter (ov2slam_amd/host/multi_view_geometry.hpp): reads the
// case file written by tests/test_gpu_p3p.py, runs ov2::p3pRansac as the front end does (LMedS, nmaxiter) and as the loop closer
// does (RANSAC, 10 x nmaxiter), then on three points, and writes each call's bool, Twc and outlier list.  File format (both ways): a
// sequence of arrays, each an int64 byte count followed by the raw bytes.
#include <cstdio>
#include "../../ov2slam_amd/host/multi_view_geometry.hpp"

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
    if (argc < 3) { fprintf(stderr, "usage: p3p_run <case> <result>\n"); return 2; }
    try {
        FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
        if (!fi || !fo) throw std::runtime_error("cannot open files");
        const std::vector<int> a = rd<int>(fi);                    // nmaxiter, seed
        const std::vector<float> e = rd<float>(fi);                // errth, fx, fy
        const std::vector<double> bv = rd<double>(fi), X = rd<double>(fi);
        const size_t n = bv.size() / 3;
        ov2::Context ctx(0);
        bool lib_ok = true;
        std::string err;
        for (int use_lmeds = 1; use_lmeds >= 0; use_lmeds--) {
            double Twc[7] = {0, 0, 0, 0, 0, 0, 1};
            std::vector<int> out;
            const int ok = ov2::p3pRansac(ctx, bv.data(), X.data(), n, use_lmeds ? a[0] : 10 * a[0], e[0], false, true, e[1], e[2], Twc, out,
                                          use_lmeds != 0, (unsigned long long)a[1], &lib_ok, &err) ? 1 : 0;
            if (!lib_ok) throw std::runtime_error("p3pRansac: " + err);
            wr(fo, &ok, 1); wr(fo, Twc, 7); wr(fo, out.data(), out.size());
        }
        double Twc[7] = {0, 0, 0, 0, 0, 0, 1};
        std::vector<int> out;
        const int ok = ov2::p3pRansac(ctx, bv.data(), X.data(), 3, a[0], e[0], false, true, e[1], e[2], Twc, out, true, 1ull, &lib_ok, &err) ? 1 : 0;
        wr(fo, &ok, 1); wr(fo, out.data(), out.size());
        std::vector<int> out2;
        if (ov2::p3pRansac(ctx, bv.data(), X.data(), n, a[0], e[0], true, true, e[1], e[2], Twc, out2, true, 1ull, &lib_ok, &err) || lib_ok)
            throw std::runtime_error("boptimize = true did not fail");
        fclose(fi); fclose(fo);
    } catch (const std::exception &ex) {
        fprintf(stderr, "%s\n", ex.what());
        return 1;
    }
    return 0;
}
