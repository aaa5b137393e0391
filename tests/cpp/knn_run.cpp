// knn_run.cpp -- test driver for the loop closer's descriptor matching through the C++ adapter (ov2slam_amd/host/loop_closer.hpp):
// reads the case file written by tests/test_gpu_knn.py, runs ov2::LoopCloser::knnMatching on one candidate and its batch overload
// (three items: the case, an item without train rows, the case with query and train swapped), and writes each vkplmids as
// (first, second) pairs.  File format (both ways): a sequence of arrays, each an int64 byte count followed by the raw bytes.
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
static void dump(FILE *f, const std::vector<std::pair<int, int>> &v)
{
    std::vector<int> kv;
    for (const auto &e : v) { kv.push_back(e.first); kv.push_back(e.second); }
    const long long nb = (long long)(kv.size() * sizeof(int));
    fwrite(&nb, 8, 1, f);
    if (nb) fwrite(kv.data(), 1, (size_t)nb, f);
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: knn_run <case> <result>\n"); return 2; }
    try {
        FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
        if (!fi || !fo) throw std::runtime_error("cannot open files");
        ov2::KnnMatchingInput in;
        in.query = rd<uint8_t>(fi);
        in.vkpids = rd<int>(fi);
        in.train = rd<uint8_t>(fi);
        in.vlmids = rd<int>(fi);
        ov2::Context ctx(0);
        const ov2::LoopCloser lc;
        std::vector<std::pair<int, int>> vkplmids{{-7, -7}};        // what the frame walk put there before (:394) stays in front
        int rc = lc.knnMatching(ctx, in.query, in.vkpids, in.train, in.vlmids, vkplmids);
        if (rc != OV2_OK) throw std::runtime_error(std::string("knnMatching: ") + ov2_last_error());
        if (vkplmids.empty() || vkplmids[0] != std::pair<int, int>(-7, -7)) throw std::runtime_error("knnMatching did not append");
        dump(fo, vkplmids);
        std::vector<int> short_ids(in.vkpids.begin(), in.vkpids.end() - 1);
        if (lc.knnMatching(ctx, in.query, short_ids, in.train, in.vlmids, vkplmids) != OV2_EINVAL)
            throw std::runtime_error("rows and ids of different lengths did not fail");
        ov2::KnnMatchingInput none = in, swapped;
        none.train.clear(); none.vlmids.clear();
        swapped.query = in.train; swapped.vkpids = in.vlmids; swapped.train = in.query; swapped.vlmids = in.vkpids;
        std::vector<std::vector<std::pair<int, int>>> vb;
        rc = lc.knnMatching(ctx, std::vector<ov2::KnnMatchingInput>{in, none, swapped}, vb);
        if (rc != OV2_OK || vb.size() != 3) throw std::runtime_error(std::string("knnMatching (batch): ") + ov2_last_error());
        if (!vb[1].empty()) throw std::runtime_error("the item without train rows returned something");
        dump(fo, vb[0]);
        dump(fo, vb[2]);
        fclose(fi); fclose(fo);
    } catch (const std::exception &ex) {
        fprintf(stderr, "%s\n", ex.what());
        return 1;
    }
    return 0;
}
