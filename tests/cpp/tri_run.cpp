// tri_run.cpp -- test driver for the keyframe triangulation through the C++ adapter (ov2slam_amd/host/mapper.hpp): reads the case
// file written by tests/test_gpu_triangulate.py, runs ov2::Mapper::triangulate and triangulateBatch (one item), and writes each
// form's status / wpt / invdepth and its action list.  File format (both ways): a sequence of arrays, each an int64 byte count
// followed by the raw bytes.
#include <cstdio>
#include "../../ov2slam_amd/host/mapper.hpp"

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
static void dump(FILE *f, const ov2::TriKeyframeOutput &o)
{
    wr(f, o.status.data(), o.status.size());
    wr(f, o.wpt.data(), o.wpt.size());
    wr(f, o.invdepth.data(), o.invdepth.size());
    std::vector<double> a;
    for (const ov2::TriMapAction &x : o.actions) {
        a.push_back((double)(int)x.op); a.push_back(x.lmid); a.push_back(x.kfid);
        a.push_back(x.wpt[0]); a.push_back(x.wpt[1]); a.push_back(x.wpt[2]); a.push_back(x.invdepth);
    }
    wr(f, a.data(), a.size());
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: tri_run <case> <result>\n"); return 2; }
    try {
        FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
        if (!fi || !fo) throw std::runtime_error("cannot open files");
        const std::vector<int> a = rd<int>(fi);                    // stereo, rect, kfid
        const std::vector<float> e = rd<float>(fi);                // fmax_reproj_err
        const std::vector<double> c = rd<double>(fi);              // K 4, iK 9, Kr 4, Tlr 7, Tcic0 7
        ov2::TriKeyframeInput in;
        in.kfid = a[2];
        const std::vector<double> twc = rd<double>(fi);
        for (int i = 0; i < 7; i++) in.Twc[i] = twc[i];
        in.lmids = rd<int>(fi);
        in.unpx = pts(rd<float>(fi));
        in.bv = rd<double>(fi);
        in.is_stereo = rd<uint8_t>(fi);
        in.runpx = pts(rd<float>(fi));
        in.rbv = rd<double>(fi);
        in.src = rd<int>(fi);
        in.src_unpx = pts(rd<float>(fi));
        in.src_bv = rd<double>(fi);
        in.src_kfid = rd<int>(fi);
        in.src_Twc = rd<double>(fi);
        in.src_Tcw = rd<double>(fi);
        ov2::Context ctx(0);
        const ov2::Mapper m(a[0] != 0, a[1] != 0, e[0], &c[0], &c[4], &c[13], &c[17], &c[24]);
        ov2::TriKeyframeOutput o;
        int rc = m.triangulate(ctx, in, o);
        if (rc != OV2_OK) throw std::runtime_error(std::string("triangulate: ") + ov2_last_error());
        dump(fo, o);
        std::vector<ov2::TriKeyframeOutput> ob;
        rc = m.triangulateBatch(ctx, std::vector<ov2::TriKeyframeInput>{in}, ob);
        if (rc != OV2_OK || ob.size() != 1) throw std::runtime_error(std::string("triangulateBatch: ") + ov2_last_error());
        dump(fo, ob[0]);
        fclose(fi); fclose(fo);
    } catch (const std::exception &ex) {
        fprintf(stderr, "%s\n", ex.what());
        return 1;
    }
    return 0;
}
