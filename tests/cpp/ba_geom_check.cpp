// ba_geom_check.cpp -- host-only check of ov2slam_amd/csrc/ba_geom.hpp (tests/test_ba_geom.py builds it with g++ against that header
// alone): every size the BA host driver hands to a launch, for n_opt = 1 .. 1024, and the layout of a lock-step batch's header
// and result block.  Prints "FAIL ..." per violated property and the
// figures the test compares; exit status 1 when anything failed.
#include "ba_geom.hpp"
#include <stdio.h>

struct Sizes { int n_kf, n_lm, n_res, n_po, nf, nfp, ldim, big, chol_hbm, lin_waves, lin_direct; };

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fails++; printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

// the sizes ba_create / xyzba_create would give the problem (no test overrides)
static Sizes sizes_of(int n_opt, int n_lm, int ldim, int n_po)
{
    Sizes D{};
    D.n_kf = n_opt + 1; D.n_lm = n_lm; D.n_res = 4 * n_lm + n_po; D.n_po = n_po; D.nf = 6 * n_opt; D.nfp = ba_nfp(n_opt); D.ldim = ldim;
    if (ldim == 1) { D.big = !ba_small_path(n_opt); D.chol_hbm = D.big; D.lin_direct = D.big && ba_lin_direct(n_opt); D.lin_waves = 4; }
    else { D.chol_hbm = ba_chol_hbm(n_opt, D.nfp); D.lin_waves = ba_xyz_lin_waves(n_opt, D.nfp); }
    return D;
}

static void check_geom(const Sizes &D, const BAGeom &g, int rows)
{
    CHECK((long long)g.ksplit * g.lm_per_split >= rows, "n_opt %d n_lm %d: %d x %d", D.nf / 6, D.n_lm, g.ksplit, g.lm_per_split);
    CHECK(g.lm_per_split % BA_TILE == 0 && g.lm_per_split >= BA_TILE, "lm_per_split %d", g.lm_per_split);
    CHECK(g.ntiles * BA_TILE == D.nfp && g.n_upper == g.ntiles * (g.ntiles + 1) / 2, "tiles %d of nfp %d", g.ntiles, D.nfp);
    CHECK((long long)g.ss_chunks * g.ss_ncol >= D.nfp && (g.ss_ncol == D.nfp || g.ss_ncol % 6 == 0), "ss_ncol %d x %d, nfp %d", g.ss_ncol, g.ss_chunks, D.nfp);
    const int grids[] = {g.lin_blocks, g.po_blocks, g.n_upper, g.ksplit, g.ss_split, g.ss_chunks, g.ws_blocks, g.bs_blocks, g.cost_blocks,
                         g.reset_blocks, g.reset_blocks_B, g.init_blocks};
    for (int v : grids) CHECK(v >= 1, "a grid of %d (n_opt %d, n_lm %d, ldim %d)", v, D.nf / 6, D.n_lm, D.ldim);
    CHECK(g.det_lin >= (D.n_lm > 0) && g.det_po >= (D.n_po > 0), "deterministic grids %d %d", g.det_lin, g.det_po);
    CHECK(g.bs_blocks <= 2048 && g.cost_blocks <= 2048, "more partial sums than BA_PART_MAX holds: %d %d", g.bs_blocks, g.cost_blocks);
}

// the layout of a lock-step batch's blocks against a restatement written out here: the parts in order, each a whole number of
// 256-byte units that holds its array
static size_t units(size_t bytes) { return (bytes + 255) / 256 * 256; }

static void check_part(const char *what, size_t off, size_t next, size_t bytes, size_t want_off)
{
    CHECK(off == want_off, "%s at %zu, expected %zu", what, off, want_off);
    CHECK(off % 256 == 0 && off + bytes <= next, "%s: %zu bytes at %zu, the next part at %zu", what, bytes, off, next);
}

static void check_out_layout(int n_kf, int n_lm, int n_res, int flags)
{
    const BAOutLayout L = ba_out_layout(n_kf, n_lm, n_res, flags);
    const size_t nk = (size_t)n_kf, nl = (size_t)n_lm, nr = (size_t)n_res;
    const size_t b_pose = units(56 * nk), b_lam = n_lm == 0 ? 256 : units(8 * nl), b_bad = units(nr);
    const size_t b_chi2 = (flags & 1) ? units(8 * nr) : 0, b_dpos = (flags & 2) ? units(nr) : 0;
    check_part("poses", L.poses, L.invdepth, 56 * nk, 0);
    check_part("invdepth", L.invdepth, L.bad_obs, 8 * nl, b_pose);
    check_part("bad_obs", L.bad_obs, L.chi2, nr, b_pose + b_lam);
    check_part("chi2", L.chi2, L.dpos, (flags & 1) ? 8 * nr : 0, b_pose + b_lam + b_bad);
    check_part("dpos", L.dpos, L.total, (flags & 2) ? nr : 0, b_pose + b_lam + b_bad + b_chi2);
    CHECK(L.total == b_pose + b_lam + b_bad + b_chi2 + b_dpos, "total %zu (%d %d %d flags %d)", L.total, n_kf, n_lm, n_res, flags);
    // the optional parts exist exactly with their flags
    CHECK((L.dpos - L.chi2 > 0) == ((flags & 1) && n_res > 0) && (L.total - L.dpos > 0) == ((flags & 2) && n_res > 0),
          "optional parts %zu %zu with flags %d (n_res %d)", L.dpos - L.chi2, L.total - L.dpos, flags, n_res);
}

static void check_batch_header(int N, size_t sizeof_ctl, size_t sizeof_dev)
{
    const BABatchHeader H = ba_batch_header(N, sizeof_ctl, sizeof_dev);
    const size_t n = (size_t)N;
    check_part("look-ahead words", H.flag, H.cnt, 4 * n, 0);
    check_part("counters", H.cnt, H.ctl, 16 * 4 * n, units(4 * n));
    check_part("control blocks", H.ctl, H.arr, sizeof_ctl * n, units(4 * n) + units(64 * n));
    check_part("device views", H.arr, H.out_base, sizeof_dev * n, units(4 * n) + units(64 * n) + units(sizeof_ctl * n));
    CHECK(H.out_base == units(4 * n) + units(64 * n) + units(sizeof_ctl * n) + units(sizeof_dev * n), "out_base %zu (N %d)", H.out_base, N);
}

int main()
{
    static const int out_cases[][3] = {{1, 0, 0}, {1, 1, 1}, {6, 40, 160}, {25, 3000, 69000}};
    for (auto &c : out_cases) for (int flags = 0; flags < 4; flags++) check_out_layout(c[0], c[1], c[2], flags);
    for (int N : {1, 11, 4096}) { check_batch_header(N, 200, 1000); check_batch_header(N, 256, 1024); check_batch_header(N, 8, 4); }
    printf("out_total_25kf_flags3 %zu\n", ba_out_layout(25, 3000, 69000, 3).total);
    int last_small = 0, first_direct = 0, last_w[5] = {0, 0, 0, 0, 0};
    for (int n = 1; n <= 1024; n++) {
        const int nf = 6 * n, nfp = ba_nfp(n);
        CHECK(nfp % BA_TILE == 0 && nfp >= nf && nfp - nf < BA_TILE && nfp <= BA_MAX_NFP, "nfp %d of nf %d", nfp, nf);
        // small path: everything the LDS-resident kernels carve up fits
        if (ba_small_path(n)) {
            CHECK(last_small == n - 1, "the small path is not one interval: %d after %d", n, last_small);
            last_small = n;
            CHECK(lin_lds_bytes(n, nfp) <= BA_LIN_LDS_MAX, "n_opt %d: lineariser %zu B", n, lin_lds_bytes(n, nfp));
            CHECK(chol_lds_bytes(nf, nfp) <= BA_CHOL_LDS_MAX, "n_opt %d: Cholesky %zu B", n, chol_lds_bytes(nf, nfp));
            CHECK(nf <= CH_MAX_LDS_N, "n_opt %d: nf %d", n, nf);
            CHECK(!ba_chol_hbm(n, nfp), "n_opt %d: small path with the HBM Cholesky", n);
        }
        // lin_direct: on exactly where the aggregated form of the large-path lineariser exceeds its limit
        CHECK(ba_lin_direct(n) == (lin_big_lds_bytes(n, false) > BA_LIN_LDS_MAX), "n_opt %d", n);
        if (ba_lin_direct(n) && !first_direct) first_direct = n;
        CHECK(lin_big_lds_bytes(n, ba_lin_direct(n)) <= BA_LIN_LDS_MAX, "n_opt %d: large-path lineariser %zu B", n, lin_big_lds_bytes(n, ba_lin_direct(n)));
        CHECK(lin_po_lds_bytes(n, ba_lin_direct(n)) <= BA_LIN_LDS_MAX, "n_opt %d: pose-only lineariser %zu B", n, lin_po_lds_bytes(n, ba_lin_direct(n)));
        // lin_waves: the largest of 4, 2, 1 that fits
        const int w = ba_xyz_lin_waves(n, nfp);
        int want = 0;
        for (int nw = 1; nw <= 4; nw *= 2) if (lin_xyz_lds_bytes(n, nfp, nw) <= BA_LIN_LDS_MAX) want = nw;
        CHECK(w == want, "n_opt %d: lin_waves %d, largest that fits %d", n, w, want);
        last_w[w] = n;
        CHECK(chol_solve_lds_bytes(nfp) <= BA_CHOL_LDS_MAX, "n_opt %d: k_chol_solve %zu B", n, chol_solve_lds_bytes(nfp));
        CHECK(backsub_lds_bytes(nfp) <= 64 * 1024, "n_opt %d: back-substitution %zu B", n, backsub_lds_bytes(nfp));

        // the launch geometry, alone (256 / 1024) and as a member of batches of 2, 11, 64 problems
        static const int n_lms[] = {0, 1, 15, 16, 17, 400, 3000, 69000};
        for (int ldim = 1; ldim <= 3; ldim += 2) {
            if (ldim == 3 && !w) continue;                              // xyzba_create refuses the problem
            for (int n_po = 0; n_po <= (ldim == 1 ? 300 : 0); n_po += 300)
                for (int n_lm : n_lms) {
                    const Sizes D = sizes_of(n, n_lm, ldim, n_po);
                    const BAGeom g = ba_geom(D, 256, 1024);
                    check_geom(D, g, ldim * n_lm);
                    CHECK(g.lin_lds <= BA_LIN_LDS_MAX && g.chol_lds <= BA_CHOL_LDS_MAX && g.ss_lds <= BA_LIN_LDS_MAX,
                          "n_opt %d ldim %d: %zu %zu %zu B", n, ldim, g.lin_lds, g.chol_lds, g.ss_lds);
                }
        }
        if (!ba_small_path(n)) continue;
        for (int N : {2, 11, 64}) {
            const int lin_cap = std::max(16, std::min(256, (768 + N - 1) / N)), schur_wgs = std::max(64, std::min(1024, (2048 + N - 1) / N));
            // the batch: this problem with each landmark count, next to the smallest and the largest small-path problem
            BAGeom each[10], G;
            int k = 0;
            for (int n_lm : n_lms) if (n_lm > 0) each[k++] = ba_geom(sizes_of(n, n_lm, 1, 0), lin_cap, schur_wgs);
            each[k++] = ba_geom(sizes_of(1, 3000, 1, 0), lin_cap, schur_wgs);
            each[k++] = ba_geom(sizes_of(69, 17, 1, 0), lin_cap, schur_wgs);
            G = each[0];
            for (int i = 1; i < k; i++) ba_geom_max(G, each[i]);
            for (int i = 0; i < k; i++) {
                const BAGeom &m = each[i];
                const int gi[][2] = {{G.lin_blocks, m.lin_blocks}, {G.po_blocks, m.po_blocks}, {G.det_lin, m.det_lin}, {G.det_po, m.det_po}, {G.ntiles, m.ntiles},
                                     {G.n_upper, m.n_upper}, {G.ksplit, m.ksplit}, {G.lm_per_split, m.lm_per_split}, {G.ss_split, m.ss_split},
                                     {G.ss_ncol, m.ss_ncol}, {G.ss_chunks, m.ss_chunks}, {G.nf, m.nf}, {G.ws_blocks, m.ws_blocks}, {G.bs_blocks, m.bs_blocks},
                                     {G.cost_blocks, m.cost_blocks}, {G.reset_blocks, m.reset_blocks}, {G.reset_blocks_B, m.reset_blocks_B}, {G.init_blocks, m.init_blocks}};
                for (auto &q : gi) CHECK(q[0] >= q[1], "batch of %d, n_opt %d: maximum %d below a member's %d", N, n, q[0], q[1]);
                const size_t gs[][2] = {{G.lin_lds, m.lin_lds}, {G.po_lds, m.po_lds}, {G.ss_lds, m.ss_lds}, {G.chol_lds, m.chol_lds}, {G.bs_lds, m.bs_lds}};
                for (auto &q : gs) CHECK(q[0] >= q[1], "batch of %d, n_opt %d: maximum %zu B below a member's %zu B", N, n, q[0], q[1]);
                CHECK(m.lin_blocks <= lin_cap, "lin_blocks %d over the cap %d", m.lin_blocks, lin_cap);
            }
            CHECK(G.lin_lds <= BA_LIN_LDS_MAX && G.chol_lds <= BA_CHOL_LDS_MAX, "batch of %d: %zu %zu B", N, G.lin_lds, G.chol_lds);
        }
    }
    const int ns = last_small;
    printf("last_small %d\nlast_small_nf %d\nlast_small_lin_lds %zu\nlast_small_chol_lds %zu\nfirst_large_nf %d\n", ns, 6 * ns,
           lin_lds_bytes(ns, ba_nfp(ns)), chol_lds_bytes(6 * ns, ba_nfp(ns)), 6 * (ns + 1));
    printf("first_lin_direct %d\nlast_lin_waves_4 %d\nlast_lin_waves_2 %d\nlast_lin_waves_1 %d\n", first_direct, last_w[4], last_w[2], last_w[1]);
    printf("failures %d\n", fails);
    return fails ? 1 : 0;
}
