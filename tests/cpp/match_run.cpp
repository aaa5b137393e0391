// match_run.cpp -- test driver for the local-map matching through the C++ adapter (ov2slam_amd/host/mapper.hpp): reads the case file
// written by tests/test_gpu_match.py, runs ov2::Mapper::matchToMap and matchToMapBatch (two items: the case and an empty keyframe),
// and writes each form's kp_lm / lm_status and its map_previd_newid as (key, value) pairs.  File format (both ways): a sequence of
// arrays, each an int64 byte count followed by the raw bytes.
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
static void dump(FILE *f, const ov2::MatchKeyframeOutput &o)
{
    wr(f, o.kp_lm.data(), o.kp_lm.size());
    wr(f, o.lm_status.data(), o.lm_status.size());
    std::vector<int> kv;
    for (const auto &e : o.map_previd_newid) { kv.push_back(e.first); kv.push_back(e.second); }
    wr(f, kv.data(), kv.size());
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: match_run <case> <result>\n"); return 2; }
    try {
        FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
        if (!fi || !fo) throw std::runtime_error("cannot open files");
        const std::vector<int> a = rd<int>(fi);                    // model, ncellsize, nb3dkps
        const std::vector<float> e = rd<float>(fi);                // fmax_proj_pxdist, fmax_desc_dist
        const std::vector<double> c = rd<double>(fi);              // K 4, img_w, img_h
        const std::vector<double> D = rd<double>(fi);
        ov2::MatchKeyframeInput in;
        in.nb3dkps = a[2];
        const std::vector<double> tcw = rd<double>(fi);
        for (int i = 0; i < 7; i++) in.Tcw[i] = tcw[i];
        in.kp_lmid = rd<int>(fi);
        in.kp_px = pts(rd<float>(fi));
        in.kp_mp = rd<int>(fi);
        in.cell_start = rd<int>(fi);
        in.cell_kp = rd<int>(fi);
        in.obs_start = rd<int>(fi);
        in.obs_kfid = rd<int>(fi);
        in.obs_kf = rd<int>(fi);
        in.obs_px = pts(rd<float>(fi));
        in.desc_start = rd<int>(fi);
        in.desc = rd<uint8_t>(fi);
        in.kf_Tcw = rd<double>(fi);
        in.lm_lmid = rd<int>(fi);
        in.lm_mp = rd<int>(fi);
        in.lm_wpt = rd<double>(fi);
        ov2::Context ctx(0);
        const double I4[4] = {1, 1, 0, 0}, I9[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, I7[7] = {0, 0, 0, 0, 0, 0, 1};
        ov2::Mapper m(false, false, 3.f, I4, I9, I4, I7, I7);
        ov2::MatchKeyframeOutput o;
        if (m.matchToMap(ctx, in, o) != OV2_EINVAL) throw std::runtime_error("matchToMap before setMatching did not fail");
        m.setMatching(a[0], &c[0], D.empty() ? nullptr : D.data(), (int)D.size(), c[4], c[5], a[1], e[0], e[1]);
        int rc = m.matchToMap(ctx, in, o);
        if (rc != OV2_OK) throw std::runtime_error(std::string("matchToMap: ") + ov2_last_error());
        dump(fo, o);
        ov2::MatchKeyframeInput empty;
        empty.cell_start.assign(in.cell_start.size(), 0);
        std::vector<ov2::MatchKeyframeOutput> ob;
        rc = m.matchToMapBatch(ctx, std::vector<ov2::MatchKeyframeInput>{in, empty}, ob);
        if (rc != OV2_OK || ob.size() != 2) throw std::runtime_error(std::string("matchToMapBatch: ") + ov2_last_error());
        if (!ob[1].map_previd_newid.empty() || !ob[1].kp_lm.empty()) throw std::runtime_error("the empty item returned something");
        dump(fo, ob[0]);
        fclose(fi); fclose(fo);
    } catch (const std::exception &ex) {
        fprintf(stderr, "%s\n", ex.what());
        return 1;
    }
    return 0;
}
