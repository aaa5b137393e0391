// loopmap_order_check.cpp -- ov2::loopLocalMapReferenceOrder (ov2slam_amd/host/loop_closer.hpp) against a literal transcription of
// the set-building walk of LoopCloser::trackLoopLocalMap (src/loop_closer.cpp:505-562) over a toy map.  No device, no library:
// also built with -fsanitize=address,undefined.  Reads walks from a file of int32 (tests/test_loopmap_order.py writes it):
//   n_walks, then per walk: lckf_kfid, n_cov, per covisibility entry (kfid, in_map, n, n lmids), n_observed, the observed lmids,
//   n_pairs, the (kpid, lmid) pairs of vkplmids
// checks that both forms leave the same vkplmids and the same local map IN THE SAME ORDER, and writes per walk: n, the local map in
// iteration order, n_pairs, the pairs, n_matched, vmatchedkpids.
#include <cstdio>
#include <map>
#include <memory>
#include <set>
#include "../../ov2slam_amd/host/loop_closer.hpp"

struct ToyKeypoint { int lmid_; };
struct ToyFrame {
    int kfid_ = 0;
    std::vector<ToyKeypoint> kps3d;
    std::set<int> observed;
    std::map<int, int> cov;
    std::vector<ToyKeypoint> getKeypoints3d() const { return kps3d; }
    bool isObservingKp(int lmid) const { return observed.count(lmid) != 0; }
    std::map<int, int> getCovisibleKfMap() const { return cov; }
};
struct ToyMap {
    std::map<int, std::shared_ptr<ToyFrame>> kfs;
    std::shared_ptr<ToyFrame> getKeyframe(int kfid) const { auto it = kfs.find(kfid); return it == kfs.end() ? nullptr : it->second; }
};

// :505-562, statement by statement
static std::vector<int> literal(const ToyMap *pmap_, const ToyFrame &newkf, const ToyFrame &lckf, std::vector<std::pair<int, int>> &vkplmids,
                                std::vector<int> &vmatchedkpids)
{
    std::unordered_set<int> set_local_lmids, set_checked_kpids;

    auto lccov_map = lckf.getCovisibleKfMap();
    lccov_map[lckf.kfid_] = 100;

    for (const auto &cokf : lccov_map) {
        int kfid = cokf.first;

        if (kfid < lckf.kfid_ - 15) {
            continue;
        } else if (kfid > lckf.kfid_ + 15) {
            break;
        }

        auto pcokf = pmap_->getKeyframe(kfid);
        if (pcokf == nullptr) {
            continue;
        }

        for (const auto &kp : pcokf->getKeypoints3d()) {
            auto it = set_checked_kpids.find(kp.lmid_);

            if (it == set_checked_kpids.end()) {
                set_checked_kpids.insert(kp.lmid_);

                if (newkf.isObservingKp(kp.lmid_)) {
                    std::pair<int, int> kplmid(kp.lmid_, kp.lmid_);
                    auto kpit = std::find(vkplmids.begin(), vkplmids.end(), kplmid);
                    if (kpit == vkplmids.end()) {
                        vkplmids.push_back(kplmid);
                    }
                } else {
                    set_local_lmids.insert(kp.lmid_);
                }
            }
        }
    }

    vmatchedkpids.clear();
    vmatchedkpids.reserve(vkplmids.size());

    for (const auto &kplmid : vkplmids) {
        vmatchedkpids.push_back(kplmid.first);
        set_local_lmids.erase(kplmid.second);
    }
    return std::vector<int>(set_local_lmids.begin(), set_local_lmids.end());
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: loopmap_order_check <walks> <result>\n"); return 2; }
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) { fprintf(stderr, "cannot open files\n"); return 2; }
    auto rd = [&]() { int v = 0; if (fread(&v, 4, 1, fi) != 1) { fprintf(stderr, "short walk file\n"); exit(2); } return v; };
    auto wr = [&](const std::vector<int> &v) { const int n = (int)v.size(); fwrite(&n, 4, 1, fo); if (n) fwrite(v.data(), 4, v.size(), fo); };
    const int n_walks = rd();
    for (int w = 0; w < n_walks; w++) {
        ToyMap map;
        ToyFrame newkf, lckf;
        lckf.kfid_ = rd();
        const int n_cov = rd();
        std::map<int, std::vector<int>> lists;                          // what the helper's caller collects, ascending keyframe id
        std::map<int, bool> in_map;
        for (int c = 0; c < n_cov; c++) {
            const int kfid = rd(), present = rd(), n = rd();
            std::vector<int> ids((size_t)n);
            for (int &v : ids) v = rd();
            if (kfid != lckf.kfid_ || present > 1) lckf.cov[kfid] = 10 + c;   // present == 2: the loop keyframe lists itself
            in_map[kfid] = present != 0;
            lists[kfid] = ids;
            if (present) {
                auto kf = std::make_shared<ToyFrame>();
                kf->kfid_ = kfid;
                for (const int v : ids) kf->kps3d.push_back(ToyKeypoint{v});
                map.kfs[kfid] = kf;
            }
        }
        for (int n = rd(); n > 0; n--) newkf.observed.insert(rd());
        std::vector<std::pair<int, int>> vk;
        for (int n = rd(); n > 0; n--) { const int a = rd(), b = rd(); vk.emplace_back(a, b); }

        std::vector<std::pair<int, int>> vk_lit = vk, vk_hlp = vk;
        std::vector<int> m_lit, m_hlp;
        const std::vector<int> lit = literal(&map, newkf, lckf, vk_lit, m_lit);
        if (!in_map.count(lckf.kfid_)) { in_map[lckf.kfid_] = false; lists[lckf.kfid_]; }   // :509: the loop keyframe is always walked
        std::vector<ov2::LoopCovisibleKeyframe> lccov;
        for (const auto &e : lists) lccov.push_back(ov2::LoopCovisibleKeyframe{e.first, in_map[e.first] ? &e.second : nullptr});
        const std::vector<int> hlp = ov2::loopLocalMapReferenceOrder(lckf.kfid_, lccov, [&](int lmid) { return newkf.isObservingKp(lmid); },
                                                                      vk_hlp, &m_hlp);
        if (lit != hlp || vk_lit != vk_hlp || m_lit != m_hlp) {
            fprintf(stderr, "walk %d: the helper and the literal walk disagree (%zu / %zu local points, %zu / %zu pairs)\n", w, hlp.size(),
                    lit.size(), vk_hlp.size(), vk_lit.size());
            return 1;
        }
        // without the optional output the same order and pairs
        std::vector<std::pair<int, int>> vk2 = vk;
        if (ov2::loopLocalMapReferenceOrder(lckf.kfid_, lccov, [&](int lmid) { return newkf.isObservingKp(lmid); }, vk2) != hlp || vk2 != vk_hlp) {
            fprintf(stderr, "walk %d: the result depends on the optional vmatchedkpids argument\n", w);
            return 1;
        }
        wr(hlp);
        std::vector<int> flat;
        for (const auto &p : vk_hlp) { flat.push_back(p.first); flat.push_back(p.second); }
        wr(flat);
        wr(m_hlp);
    }
    fclose(fi); fclose(fo);
    return 0;
}
