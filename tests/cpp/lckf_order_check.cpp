// lckf_order_check.cpp -- runs ov2::retainBestReferenceOrder (ov2slam_amd/host/loop_closer.hpp: the literal std::nth_element /
// std::partition of KeyPointsFilter::retainBest) on response lists read from a file and writes what it leaves.  No device is needed:
// tests/test_lckf_reference.py compares the kept SET with the histogram rule of tests/lckf_ref.py.
// Input:  int32 n_lists, then per list int32 retain, int32 n, n response bytes (corner i is (x, y) = (i & 0x7fff, i >> 15)).
// Output: per list int32 n_kept, then n_kept int32 indices in the order the helper leaves them.
#include <cstdio>
#include <cstdlib>
#include "../../ov2slam_amd/host/loop_closer.hpp"

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: lckf_order_check <lists> <result>\n"); return 2; }
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) { fprintf(stderr, "cannot open files\n"); return 1; }
    int n_lists = 0;
    if (fread(&n_lists, 4, 1, fi) != 1) return 1;
    for (int l = 0; l < n_lists; l++) {
        int retain = 0, n = 0;
        if (fread(&retain, 4, 1, fi) != 1 || fread(&n, 4, 1, fi) != 1 || n < 0) return 1;
        std::vector<uint8_t> resp((size_t)n);
        if (n && fread(resp.data(), 1, (size_t)n, fi) != (size_t)n) return 1;
        std::vector<ov2::LckfCorner> kps((size_t)n);
        for (int i = 0; i < n; i++) kps[(size_t)i] = ov2::LckfCorner{(int16_t)(i & 0x7fff), (int16_t)(i >> 15), resp[(size_t)i]};
        ov2::retainBestReferenceOrder(kps, retain);
        const int nk = (int)kps.size();
        fwrite(&nk, 4, 1, fo);
        for (const ov2::LckfCorner &k : kps) {
            const int idx = (int)k.x | ((int)k.y << 15);
            if (idx < 0 || idx >= n || resp[(size_t)idx] != k.response) { fprintf(stderr, "list %d: a corner that was not in the input\n", l); return 1; }
            fwrite(&idx, 4, 1, fo);
        }
    }
    fclose(fi); fclose(fo);
    return 0;
}
