// pose_adapters.cpp -- test driver for the per-frame pose through the C++ adapters (ov2slam_amd/host/visual_front_end.hpp:
// ov2::computePose, single and batched; ov2slam_amd/host/multi_view_geometry.hpp: ov2::ceresPnPFused): reads the case file written
// by tests/test_gpu_computepose.py, runs the frame alone, then twice in a batch, then the fused PnP on the same arrays, and
// writes what each returned.  File format (both ways): a sequence of arrays, each an int64 byte count followed by the raw bytes.
#include <cstdio>
#include "../../ov2slam_amd/host/visual_front_end.hpp"
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

static void wr_pose(FILE *fo, int rc, const ov2::ComputePoseOutput &o)
{
    const int head[7] = {rc, o.r.action, o.r.p3p_req_out, o.r.n_removed_p3p, o.r.n_outliers_pnp, o.r.p3p_status, o.r.p3p_best_row};
    wr(fo, head, 7); wr(fo, o.r.Twc, 7); wr(fo, o.removed.data(), o.removed.size());
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: pose_adapters <case> <result>\n"); return 2; }
    try {
        FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
        if (!fi || !fo) throw std::runtime_error("cannot open files");
        const std::vector<int> a = rd<int>(fi);                    // nransac_iter, seed, do_p3p, p3p_req, mono, apply_l2
        const std::vector<float> e = rd<float>(fi);                // fransac_err, robust_mono_th, fx, fy, cx, cy
        ov2::ComputePoseInput in;
        in.unpx = rd<double>(fi); in.wpt = rd<double>(fi); in.bv = rd<double>(fi);
        const std::vector<double> Twc = rd<double>(fi);
        in.scale = rd<int>(fi);
        for (int i = 0; i < 7; i++) in.Twc[i] = Twc[i];
        in.seed = (unsigned long long)a[1]; in.do_p3p = a[2] != 0; in.p3p_req = a[3] != 0;
        ov2::ComputePoseParams P;
        P.nransac_iter = a[0]; P.fransac_err = e[0]; P.robust_mono_th = e[1]; P.mono = a[4] != 0; P.apply_l2_after_robust = a[5] != 0;
        P.fx = e[2]; P.fy = e[3]; P.cx = e[4]; P.cy = e[5];
        ov2::Context ctx(0);
        ov2::ComputePoseOutput one;
        const int rc1 = ov2::computePose(ctx, P, in, one);
        wr_pose(fo, rc1, one);
        std::vector<ov2::ComputePoseOutput> two;
        const int rc2 = ov2::computePose(ctx, P, std::vector<ov2::ComputePoseInput>(2, in), two);
        for (const auto &o : two) wr_pose(fo, rc2, o);
        double T[7];
        for (int i = 0; i < 7; i++) T[i] = Twc[i];
        std::vector<int> out;
        bool lib_ok = true;
        std::string err;
        const int ok = ov2::ceresPnPFused(ctx, in.unpx.data(), in.wpt.data(), in.scale.data(), in.scale.size(), T, 5, e[1], true, a[5] != 0,
                                          e[2], e[3], e[4], e[5], out, &lib_ok, &err) ? 1 : 0;
        if (!lib_ok) throw std::runtime_error("ceresPnPFused: " + err);
        wr(fo, &ok, 1); wr(fo, T, 7); wr(fo, out.data(), out.size());
        fclose(fi); fclose(fo);
    } catch (const std::exception &ex) {
        fprintf(stderr, "%s\n", ex.what());
        return 1;
    }
    return 0;
}
