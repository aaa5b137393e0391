// kfreq_sort_check.cpp -- stand-alone check of the host-only helpers of the frame-versus-keyframe adapter
// (ov2slam_amd/host/visual_front_end.hpp: detail::sortKeyframeByLmid, detail::packFkf).  It calls nothing of the library, so it
// links without it; tests/test_kfreq_host_helpers.py builds it with -fsanitize=address,undefined and runs it on the CPU.
#include <cstdio>
#include <cstdlib>
#include "../../ov2slam_amd/host/visual_front_end.hpp"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main()
{
    unsigned long long state = 12345;
    auto next = [&state]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(state >> 33); };
    for (int n : {0, 1, 2, 7, 300, 2048}) {
        std::vector<int> lmid((size_t)n);
        std::vector<ov2::Point2f> unpx((size_t)n);
        for (int i = 0; i < n; i++) { lmid[i] = 3 * i + 1; unpx[i] = ov2::Point2f((float)(3 * i + 1), (float)-i); }
        for (int i = n - 1; i > 0; i--) {                           // shuffle both alike
            const int j = (int)(next() % (unsigned)(i + 1));
            std::swap(lmid[i], lmid[j]); std::swap(unpx[i], unpx[j]);
        }
        std::vector<int> sl;
        std::vector<float> su;
        CHECK(ov2::detail::sortKeyframeByLmid(lmid, unpx, sl, su));
        CHECK(sl.size() == (size_t)n && su.size() == 2 * (size_t)n);
        for (int i = 0; i < n; i++) CHECK(sl[i] == 3 * i + 1 && su[2 * i] == (float)(3 * i + 1) && su[2 * i + 1] == (float)-i);
        if (n >= 2) {
            std::vector<int> dup = lmid;
            dup[0] = dup[n - 1];
            CHECK(!ov2::detail::sortKeyframeByLmid(dup, unpx, sl, su));          // a repeated id
            unpx.pop_back();
            CHECK(!ov2::detail::sortKeyframeByLmid(lmid, unpx, sl, su));         // arrays of different length
        }
    }
    ov2::FrameVsKeyframe f;
    ov2::detail::FkfPacked p;
    CHECK(ov2::detail::packFkf(f, p) && p.item.n_cur == 0 && p.item.n_kf == 0 && p.item.cur_lmid && p.item.kf_unpx);   // empty: no NULL arrays
    f.cur_lmid = {5, 2, 9}; f.cur_px.resize(3); f.cur_unpx.resize(3); f.cur_bv.resize(9); f.cur_is3d.resize(3);
    f.kf_lmid = {9, 2}; f.kf_unpx = {ov2::Point2f(9.f, 0.f), ov2::Point2f(2.f, 0.f)};
    CHECK(ov2::detail::packFkf(f, p) && p.item.n_cur == 3 && p.item.n_kf == 2 && p.item.kf_lmid[0] == 2 && p.item.kf_unpx[2] == 9.f);
    CHECK(p.item.cur_lmid == f.cur_lmid.data() && p.item.noccupcells == -1 && p.item.nb3dkps == -1);
    f.cur_bv.resize(8);
    CHECK(!ov2::detail::packFkf(f, p));
    std::vector<ov2::detail::FkfPacked> packed;
    std::vector<ov2_fkf_item> items;
    f.cur_bv.resize(9);
    CHECK(ov2::detail::packFkfBatch({f, ov2::FrameVsKeyframe(), f}, packed, items) && items.size() == 3 && items[2].kf_lmid == packed[2].kf_lmid.data());
    printf("kfreq_sort_check ok\n");
    return 0;
}
