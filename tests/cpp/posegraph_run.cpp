// posegraph_run.cpp -- test driver for the pose-graph solve through the C++ adapter (ov2slam_amd/host/optimizer.hpp): reads the case
// file written by tests/test_gpu_posegraph.py (poses, pose_const, edge_i, edge_j, edge_T, full), fills a FlatPoseGraph the way the
// reference's loops add their blocks, runs Optimizer::solvePoseGraph and writes the bool, the termination and poses_out.  File
// format (both ways): a sequence of arrays, each an int64 byte count followed by the raw bytes.
#include <cstdio>
#include <stdexcept>
#include "../../ov2slam_amd/host/optimizer.hpp"

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
    if (argc < 3) { fprintf(stderr, "usage: posegraph_run <case> <result>\n"); return 2; }
    try {
        FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
        if (!fi || !fo) throw std::runtime_error("cannot open files");
        const std::vector<double> poses = rd<double>(fi);
        const std::vector<uint8_t> pose_const = rd<uint8_t>(fi);
        const std::vector<int> ei = rd<int>(fi), ej = rd<int>(fi);
        const std::vector<double> eT = rd<double>(fi);
        const std::vector<int> full = rd<int>(fi);
        ov2::FlatPoseGraph pg;
        for (size_t k = 0; k < pose_const.size(); k++) pg.addPose(poses.data() + 7 * k, pose_const[k] != 0);
        for (size_t e = 0; e < ei.size(); e++) pg.addEdge(ei[e], ej[e], eT.data() + 7 * e);
        ov2::Context ctx(0);
        ov2::Optimizer opt(5.9915, true);
        std::vector<double> out;
        int term = -1;
        const int ok = opt.solvePoseGraph(ctx, pg, full[0] != 0, out, &term) ? 1 : 0;
        if (!ok) throw std::runtime_error(std::string("solvePoseGraph: ") + ov2_last_error());
        wr(fo, &ok, 1); wr(fo, &term, 1); wr(fo, out.data(), out.size());
        fclose(fi); fclose(fo);
    } catch (const std::exception &ex) {
        fprintf(stderr, "%s\n", ex.what());
        return 1;
    }
    return 0;
}
