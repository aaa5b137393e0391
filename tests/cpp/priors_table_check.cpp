// priors_table_check.cpp -- stand-alone check of the host-only helpers of the prior adapters (ov2slam_amd/host/visual_front_end.hpp:
// detail::packKltPriors; ov2slam_amd/host/feature_tracker.hpp: detail::priorGridCells, detail::buildCellTable,
// detail::packStereoPriors).  It calls nothing of the library, so it links without it; tests/test_priors_host_helpers.py builds it
// with -fsanitize=address,undefined and runs it on the CPU.
#include <cstdio>
#include <cstdlib>
#include "../../ov2slam_amd/host/feature_tracker.hpp"
#include "../../ov2slam_amd/host/visual_front_end.hpp"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main()
{
    unsigned long long state = 2024;
    auto next = [&state]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(state >> 33); };
    // Frame's grid: ceil in float, as frame.cpp:41-43
    CHECK(ov2::detail::priorGridCells(752, 480, 35) == 22 * 14);
    CHECK(ov2::detail::priorGridCells(768, 512, 32) == 24 * 16);
    CHECK(ov2::detail::priorGridCells(1, 1, 35) == 1);
    CHECK(ov2::detail::priorGridCells(0, 480, 35) == 0 && ov2::detail::priorGridCells(752, 480, 0) == 0 && ov2::detail::priorGridCells(752, -1, 35) == 0);
    CHECK(ov2::detail::priorGridCells(1e9, 480, 35) == 0);

    ov2::StereoPriorsParams P;
    P.rightcam.img_w = 752; P.rightcam.img_h = 480; P.ncellsize = 35;
    const size_t ncells = 22 * 14;
    for (int n : {0, 1, 2, 65, 308, 2048}) {
        ov2::StereoPriorsInput f;
        f.px.resize((size_t)n); f.unpx.resize((size_t)n); f.bv.assign(3 * (size_t)n, 0.5); f.wpt.assign(3 * (size_t)n, 1.0); f.state.assign((size_t)n, 1);
        f.grid.assign(ncells, std::vector<int>());
        std::vector<int> cell_of((size_t)n);
        for (int i = n - 1; i >= 0; i--) {                          // rows enter their cells in descending order: not the keypoint order
            const size_t c = next() % ncells;
            f.grid[c].push_back(i); cell_of[(size_t)i] = (int)c;
        }
        ov2::detail::StereoPriorsPacked p;
        CHECK(ov2::detail::packStereoPriors(P, f, p));
        CHECK(p.item.n == n && p.cell_start.size() == ncells + 1 && p.cell_start[0] == 0 && p.cell_start[ncells] == n && p.cell_kp.size() == (size_t)n);
        CHECK(p.item.cell_start == p.cell_start.data() && p.item.cell_kp != nullptr && p.item.px != nullptr && p.item.state != nullptr);
        std::vector<int> seen((size_t)n, 0);
        for (size_t c = 0; c < ncells; c++) {
            CHECK(p.cell_start[c] <= p.cell_start[c + 1] && (size_t)(p.cell_start[c + 1] - p.cell_start[c]) == f.grid[c].size());
            for (int j = p.cell_start[c]; j < p.cell_start[c + 1]; j++) {
                const int k = p.cell_kp[(size_t)j];
                CHECK(k >= 0 && k < n && cell_of[(size_t)k] == (int)c && k == f.grid[c][(size_t)(j - p.cell_start[c])]);   // the cell's own order
                seen[(size_t)k]++;
            }
        }
        for (int i = 0; i < n; i++) CHECK(seen[(size_t)i] == 1);
        if (n >= 2) {
            ov2::StereoPriorsInput g = f;
            g.grid[(size_t)cell_of[0]].push_back(n);                 // a row outside the keypoints
            CHECK(!ov2::detail::packStereoPriors(P, g, p));
            g = f; g.grid[3].push_back(-1);
            CHECK(!ov2::detail::packStereoPriors(P, g, p));
            g = f; g.grid.pop_back();                                // a grid of another size
            CHECK(!ov2::detail::packStereoPriors(P, g, p));
            g = f; g.bv.pop_back();                                  // arrays of different length
            CHECK(!ov2::detail::packStereoPriors(P, g, p));
            g = f; g.state.push_back(0);
            CHECK(!ov2::detail::packStereoPriors(P, g, p));
        }
        ov2::StereoPriorsParams Pr = P;
        Pr.rect = true;
        ov2::StereoPriorsInput h = f;
        h.grid.clear();                                              // rectified pairs need no grid
        CHECK(ov2::detail::packStereoPriors(Pr, h, p) && p.cell_start.size() == ncells + 1 && p.cell_start[ncells] == 0 && p.item.cell_kp != nullptr);
        CHECK(!ov2::detail::packStereoPriors(P, h, p));

        ov2::KltPriorsInput k;
        k.px.resize((size_t)n); k.is3d.assign((size_t)n, 1); k.wpt.assign(3 * (size_t)n, 2.0);
        ov2_klt_priors_item it{};
        CHECK(ov2::detail::packKltPriors(k, it) && it.n == n && it.px && it.is3d && it.wpt && it.Tcw == k.Tcw);
        if (n) CHECK(it.px == &k.px[0].x && it.wpt == k.wpt.data());
        k.wpt.push_back(0.);
        CHECK(!ov2::detail::packKltPriors(k, it));
    }
    ov2::ProjectionCamera cam;
    cam.D = {0.1, 0.2, 0.3, 0.4};
    const ov2_klt_priors_params kp = ov2::detail::kltPriorsParams(cam, true);
    CHECK(kp.nD == 4 && kp.D == cam.D.data() && kp.klt_use_prior == 1);
    P.rightcam.D.clear(); P.Tcic0[0] = -0.11;
    const ov2_stereo_priors_params sp = ov2::detail::stereoPriorsParams(P);
    CHECK(sp.nD == 0 && sp.D == nullptr && sp.Tcic0[0] == -0.11 && sp.Tcic0[6] == 1. && sp.ncellsize == 35 && sp.rect == 0);
    printf("priors_table_check ok\n");
    return 0;
}
