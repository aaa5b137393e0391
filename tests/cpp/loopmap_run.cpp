// loopmap_run.cpp -- test driver for the loop local-map tracking through the C++ adapter (ov2slam_amd/host/loop_closer.hpp): reads the
// case file written by tests/test_gpu_loopmap.py, runs ov2::LoopCloser::trackLoopLocalMap in its single and its batch form (two
// items: the case and an empty candidate) on the vkplmids the walk left, and writes each form's vkplmids as (kpid, lmid) pairs with
// its kp_lm / lm_status.  File format (both ways): a sequence of arrays, each an int64 byte count followed by the raw bytes.
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
static void dump(FILE *f, const std::vector<std::pair<int, int>> &vk, const ov2::LoopMapOutput &o)
{
    std::vector<int> kv;
    for (const auto &e : vk) { kv.push_back(e.first); kv.push_back(e.second); }
    wr(f, kv.data(), kv.size());
    wr(f, o.kp_lm.data(), o.kp_lm.size());
    wr(f, o.lm_status.data(), o.lm_status.size());
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: loopmap_run <case> <result>\n"); return 2; }
    try {
        FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
        if (!fi || !fo) throw std::runtime_error("cannot open files");
        const std::vector<int> a = rd<int>(fi);                    // model, ncellsize
        const std::vector<float> e = rd<float>(fi);                // fmaxprojerr, fdistratio
        const std::vector<double> c = rd<double>(fi);              // K 4, img_w, img_h
        const std::vector<double> D = rd<double>(fi);
        ov2::LoopMapInput in;
        const std::vector<double> tcw = rd<double>(fi);
        for (int i = 0; i < 7; i++) in.Tcw[i] = tcw[i];
        in.kp_lmid = rd<int>(fi);
        in.kp_px = pts(rd<float>(fi));
        in.kp_mp = rd<int>(fi);
        in.kp_matched = rd<uint8_t>(fi);
        in.cell_start = rd<int>(fi);
        in.cell_kp = rd<int>(fi);
        in.obs_start = rd<int>(fi);
        in.obs_kfid = rd<int>(fi);
        in.desc_start = rd<int>(fi);
        in.desc = rd<uint8_t>(fi);
        in.lm_lmid = rd<int>(fi);
        in.lm_mp = rd<int>(fi);
        in.lm_wpt = rd<double>(fi);
        const std::vector<int> walk = rd<int>(fi);                 // vkplmids after the walk, flat
        std::vector<std::pair<int, int>> vk0;
        for (size_t i = 0; i + 1 < walk.size(); i += 2) vk0.emplace_back(walk[i], walk[i + 1]);

        ov2::Context ctx(0);
        ov2::LoopCloser lc;
        ov2::LoopMapOutput o;
        std::vector<std::pair<int, int>> vk = vk0;
        if (lc.trackLoopLocalMap(ctx, in, vk, &o) != OV2_EINVAL || vk != vk0 || !o.kp_lm.empty())
            throw std::runtime_error("trackLoopLocalMap before setLoopMapMatching did not fail cleanly");
        lc.setLoopMapMatching(a[0], &c[0], D.empty() ? nullptr : D.data(), (int)D.size(), c[4], c[5], a[1], e[0], e[1]);
        ov2::LoopMapInput bad = in;
        if (!bad.lm_mp.empty()) bad.lm_mp[0] = (int)in.obs_start.size();      // outside the map-point table
        if (!bad.lm_mp.empty() && (lc.trackLoopLocalMap(ctx, bad, vk, &o) != OV2_EINVAL || vk != vk0 || !o.kp_lm.empty()))
            throw std::runtime_error("a rejected call changed vkplmids");
        int rc = lc.trackLoopLocalMap(ctx, in, vk, &o);
        if (rc != OV2_OK) throw std::runtime_error(std::string("trackLoopLocalMap: ") + ov2_last_error());
        dump(fo, vk, o);
        ov2::LoopMapInput empty;
        empty.cell_start.assign(in.cell_start.size(), 0);
        std::vector<std::vector<std::pair<int, int>>> vkb{vk0, {{7, 8}}};
        std::vector<ov2::LoopMapOutput> ob;
        rc = lc.trackLoopLocalMap(ctx, std::vector<ov2::LoopMapInput>{in, empty}, vkb, &ob);
        if (rc != OV2_OK || ob.size() != 2 || vkb.size() != 2) throw std::runtime_error(std::string("trackLoopLocalMap (batch): ") + ov2_last_error());
        if (vkb[1] != std::vector<std::pair<int, int>>{{7, 8}} || !ob[1].kp_lm.empty()) throw std::runtime_error("the empty item returned something");
        dump(fo, vkb[0], ob[0]);
        fclose(fi); fclose(fo);
    } catch (const std::exception &ex) {
        fprintf(stderr, "%s\n", ex.what());
        return 1;
    }
    return 0;
}
