// ba_geom.hpp -- the ONE place that knows the sizes of the device bundle adjustment: tile and panel constants, the dynamic-LDS
// byte count of every kernel that carves up dynamic LDS, which path a problem takes, and the grids of the LM loop's launches.
// Plain C++ (no HIP types, no context): ba.hip includes it ahead of the kernels, tests/cpp/ba_geom_check.cpp builds it alone.
// A kernel whose LDS layout changes changes its function here, and nothing else on the host.  The two blocks of a lock-step batch
// (header, results) are laid out here as well: k_ba_gather_B writes the result block by the function the host reads it by.
#pragma once
#include <stddef.h>
#include <algorithm>

#if defined(__HIPCC__)
#define BA_HD __host__ __device__
#else
#define BA_HD
#endif

#define BA_TILE 32
#define BA_MAX_NFP 6144     // 1024 optimised keyframes: H, G, S are dense nfp x nfp doubles (302 MB each at the cap)
#define LIN_NRED 35         // per-landmark sums of the inverse-depth lineariser, reduced through a per-wave 35 x 33 LDS transpose
#define LIN_RED (LIN_NRED * 33)
#define CH_NB 32
#define CH_LDP 33           // padded leading dimension (doubles) of the LDS panel rows
#define CH_MAX_LDS_N 415    // k_ba_cholesky (512 threads, six panel wavefronts): the right-hand side rides as a panel row, n - 32 + 1 <= 384; larger: HBM path
#define SS_WAVES 8          // wavefronts per work-group of k_ba_schur_sparse
// dynamic LDS a launch may ask for: the 160 KB of a gfx950 work-group less the kernel's static __shared__ arrays, rounded up
// to whole KB -- the linearisers' reduction buffers (64 B), the Cholesky's 32 x 33 reduction tile + pivots (8.8 KB)
#define BA_LIN_LDS_MAX ((size_t)159 * 1024)
#define BA_CHOL_LDS_MAX ((size_t)150 * 1024)

// reduced-system order padded to whole tiles
static inline int ba_nfp(int n_opt) { return std::max(BA_TILE, (6 * n_opt + BA_TILE - 1) / BA_TILE * BA_TILE); }

// ---------------------------------------------------------------------------------- dynamic LDS, bytes, per kernel
// k_ba_linearize<false> / k_ba_linearize_B: two W rows per wavefront, observer blocks + F^T b, four per-wave anchor-observer caches,
// four reduction scratches
static inline size_t lin_lds_bytes(int n_opt, int nfp) { return 8 * (8 * (size_t)nfp + (size_t)n_opt * 27 + 4 * (size_t)n_opt * 21 + 4 * (size_t)LIN_RED) + 64; }
// k_ba_linearize<true>: observer blocks + F^T b (none with lin_direct) and the reduction scratches
static inline size_t lin_big_lds_bytes(int n_opt, bool direct) { return 8 * ((direct ? 0 : (size_t)n_opt * 27) + 4 * (size_t)LIN_RED) + 64; }
// k_ba_linearize_xyz: three W rows per wavefront, observer blocks + F^T b
static inline size_t lin_xyz_lds_bytes(int n_opt, int nfp, int waves) { return 8 * (3 * (size_t)waves * nfp + (size_t)n_opt * 27) + 64; }
// k_ba_linearize_po: observer blocks + F^T b (none with lin_direct)
static inline size_t lin_po_lds_bytes(int n_opt, bool direct) { return (direct ? 0 : (size_t)n_opt * 27 * 8) + 16; }
// k_ba_cholesky: diagonal block, solution vector, panel (rows rounded up to whole 16-row MFMA tiles: the trailing update reads its
// operand rows unpredicated), reciprocal pivots
static inline size_t chol_lds_bytes(int nf, int nfp) { return 8 * ((size_t)CH_NB * CH_LDP + 2 * (size_t)nfp + (size_t)((std::max(0, nf - CH_NB) + 15) & ~15) * CH_LDP) + 64; }
// k_chol_solve: scratch block + the solution vector
static inline size_t chol_solve_lds_bytes(int nfp) { return 8 * ((size_t)CH_NB * CH_LDP + (size_t)nfp) + 64; }
// k_ba_schur_sparse: ncol columns of the row block + per-wavefront staging (64 slot blocks and their columns)
static inline size_t schur_sparse_lds_bytes(int ncol) { return 8 * (6 * (size_t)ncol + (size_t)SS_WAVES * 64 * 6) + 4 * (size_t)SS_WAVES * 64 + 64; }
// k_ba_backsub / k_ba_backsub_xyz: the pose step
static inline size_t backsub_lds_bytes(int nfp) { return (size_t)nfp * 8; }

// ---------------------------------------------------------------------------------- which path
// the reduced system outgrows the one-work-group LDS Cholesky: the multi-kernel factorisation on HBM (k_chol_*)
static inline bool ba_chol_hbm(int n_opt, int nfp) { return chol_lds_bytes(6 * n_opt, nfp) > BA_CHOL_LDS_MAX || 6 * n_opt > CH_MAX_LDS_N; }
// inverse-depth form: dense W with the LDS-aggregating lineariser and the LDS Cholesky -- up to 69 optimised keyframes (nf = 414;
// CH_MAX_LDS_N is the first of the three bounds to give); beyond: sparse W + HBM Cholesky (BADev::big)
static inline bool ba_small_path(int n_opt) { const int nfp = ba_nfp(n_opt); return lin_lds_bytes(n_opt, nfp) <= BA_LIN_LDS_MAX && !ba_chol_hbm(n_opt, nfp); }
// large path: the observer blocks no longer fit the work-group's LDS either (from 583 optimised keyframes) -- global atomics
static inline bool ba_lin_direct(int n_opt) { return lin_big_lds_bytes(n_opt, false) > BA_LIN_LDS_MAX; }
// 3-D point form: wavefronts per lineariser work-group, the largest of 4, 2, 1 whose W rows fit: up to 202, 320, 451 optimised
// keyframes (0: none does)
static inline int ba_xyz_lin_waves(int n_opt, int nfp)
{
    for (int nw = 4; nw >= 1; nw >>= 1) if (lin_xyz_lds_bytes(n_opt, nfp, nw) <= BA_LIN_LDS_MAX) return nw;
    return 0;
}

// ---------------------------------------------------------------------------------- launch geometry of the LM loop
struct BAGeom {
    int lin_blocks, po_blocks, det_lin, det_po;         // linearisers (det_*: the one-wavefront work-groups of the deterministic mode)
    int ntiles, n_upper, ksplit, lm_per_split;          // k_ba_schur_gemm: n_upper x ksplit work-groups
    int ss_split, ss_ncol, ss_chunks;                   // k_ba_schur_sparse: n_opt * ss_split x ss_chunks
    int nf;                                             // k_ba_assemble: (nf + 255) / 256 x nf
    int ws_blocks, bs_blocks, cost_blocks;              // 3-D point prep / back-substitution / cost; inverse-depth back-substitution; cost
    int reset_blocks, reset_blocks_B, init_blocks;      // k_ba_reset, k_ba_reset_B (its grid never counted the landmarks), k_ba_init
    size_t lin_lds, po_lds, ss_lds, chol_lds, bs_lds;   // dynamic LDS of the lineariser in the problem's form, k_ba_linearize_po,
                                                        // k_ba_schur_sparse, k_ba_cholesky or k_chol_solve, the back-substitution
};

// D: the sizes of a BADev (n_kf, n_lm, n_res, n_po, nf, nfp, ldim, big, chol_hbm, lin_waves, lin_direct).  lin_cap: most
// lineariser work-groups; schur_wgs: the k_ba_schur_gemm work-groups to aim for (a problem alone spreads over the whole chip:
// 256 / 1024; a batch shares it); schur_chunk: OV2_OPT_BA_SCHUR_CHUNK (columns, 0 = auto).
template <class Sizes>
static inline BAGeom ba_geom(const Sizes &D, int lin_cap, int schur_wgs, int schur_chunk = 0)
{
    BAGeom g;
    const int n_opt = D.nf / 6;
    const bool direct = D.big && D.lin_direct;
    g.lin_blocks = std::max(1, std::min(lin_cap, (D.n_lm + 15) / 16));     // 16 landmarks per work-group (512 at a time: two per CU -- measured 15 % slower)
    g.po_blocks = std::max(1, std::min(256, (D.n_po + 255) / 256));
    g.det_lin = D.n_lm > 0 ? std::max(1, std::min(128, (D.n_lm + 15) / 16)) : 0;
    g.det_po = D.n_po > 0 ? std::max(1, std::min(32, (D.n_po + 63) / 64)) : 0;
    // rows of the W^T C W contraction: landmarks, or the 3 pseudo-rows per point of Wp (ldim 3)
    const int rows = D.ldim == 3 ? 3 * D.n_lm : D.n_lm;
    g.ntiles = D.nfp / BA_TILE; g.n_upper = g.ntiles * (g.ntiles + 1) / 2;
    g.ksplit = std::max(1, std::min(64, (schur_wgs + g.n_upper - 1) / g.n_upper));
    g.lm_per_split = std::max(BA_TILE, ((rows + g.ksplit - 1) / g.ksplit + BA_TILE - 1) / BA_TILE * BA_TILE);
    g.ksplit = std::max(1, (rows + g.lm_per_split - 1) / g.lm_per_split);
    // k_ba_schur_sparse: ~512 work-groups; the column chunk of the row block kept in LDS: all of it up to 2040 columns (340 pose
    // blocks), else that many per chunk
    g.ss_split = std::max(1, (512 + std::max(1, n_opt) - 1) / std::max(1, n_opt));
    g.ss_ncol = D.nfp <= 2048 ? D.nfp : 2040;
    if (schur_chunk >= 6) g.ss_ncol = std::min(g.ss_ncol, schur_chunk / 6 * 6);
    g.ss_chunks = (D.nfp + g.ss_ncol - 1) / g.ss_ncol;
    g.nf = D.nf;
    g.ws_blocks = std::max(1, std::min(512, std::max((D.n_lm + 3) / 4, (D.n_po + 255) / 256)));
    // inverse-depth form: 16 landmarks per work-group pass in the back-substitution, 8 in the cost kernel -- one pass each when the grid allows
    g.bs_blocks = std::max(1, std::min(2048, (D.n_lm + 15) / 16));
    g.cost_blocks = std::max(1, std::min(2048, std::max((D.n_lm + 7) / 8, (D.n_po + 255) / 256)));
    // (the reset kernels walk every array with a grid-stride loop: either grid gives the same state)
    const size_t reset_n = (size_t)std::max(D.n_res, D.nfp * D.nfp);
    g.reset_blocks = std::max(1, (int)std::min<size_t>(256, (std::max(reset_n, (size_t)D.n_lm) + 1023) / 1024));
    g.reset_blocks_B = std::max(1, (int)std::min<size_t>(256, (reset_n + 1023) / 1024));
    g.init_blocks = (int)std::min<size_t>(1024, (std::max<size_t>(std::max<size_t>(D.n_kf, D.nfp), (size_t)D.n_lm * D.ldim) + 255) / 256);
    g.lin_lds = D.big ? lin_big_lds_bytes(n_opt, direct) : D.ldim == 3 ? lin_xyz_lds_bytes(n_opt, D.nfp, D.lin_waves) : lin_lds_bytes(n_opt, D.nfp);
    g.po_lds = lin_po_lds_bytes(n_opt, direct);
    g.ss_lds = schur_sparse_lds_bytes(g.ss_ncol);
    g.chol_lds = D.chol_hbm ? chol_solve_lds_bytes(D.nfp) : chol_lds_bytes(D.nf, D.nfp);
    g.bs_lds = backsub_lds_bytes(D.nfp);
    return g;
}

// per-field maximum: the grids and LDS bytes of a lock-step batch are the largest any of its problems needs (each problem's view
// still gets the Schur split of its own geometry)
static inline void ba_geom_max(BAGeom &a, const BAGeom &b)
{
    int BAGeom::*const gi[] = {&BAGeom::lin_blocks, &BAGeom::po_blocks, &BAGeom::det_lin, &BAGeom::det_po, &BAGeom::ntiles, &BAGeom::n_upper,
                               &BAGeom::ksplit, &BAGeom::lm_per_split, &BAGeom::ss_split, &BAGeom::ss_ncol, &BAGeom::ss_chunks, &BAGeom::nf,
                               &BAGeom::ws_blocks, &BAGeom::bs_blocks, &BAGeom::cost_blocks, &BAGeom::reset_blocks, &BAGeom::reset_blocks_B, &BAGeom::init_blocks};
    size_t BAGeom::*const gs[] = {&BAGeom::lin_lds, &BAGeom::po_lds, &BAGeom::ss_lds, &BAGeom::chol_lds, &BAGeom::bs_lds};
    for (auto f : gi) a.*f = std::max(a.*f, b.*f);
    for (auto f : gs) a.*f = std::max(a.*f, b.*f);
}

// ---------------------------------------------------------------------------------- the blocks of a lock-step batch (ba_local.hpp)
static inline BA_HD size_t ba_up256(size_t v) { return (v + 255) & ~(size_t)255; }

// one problem's slot of the batch's result block: poses | inverse depths | outlier verdicts [| chi2] [| depth flags], offsets in
// bytes, 256-byte parts (a problem without landmarks keeps one part of inverse depths); out_flags 1: + chi2, 2: + depth flags --
// a part that is not there is empty, so its offset is the next part's
struct BAOutLayout { size_t poses, invdepth, bad_obs, chi2, dpos, total; };
static inline BA_HD BAOutLayout ba_out_layout(int n_kf, int n_lm, int n_res, int out_flags)
{
    const size_t nk = (size_t)(n_kf > 0 ? n_kf : 0), nl = (size_t)(n_lm > 1 ? n_lm : 1), nr = (size_t)(n_res > 0 ? n_res : 0);
    BAOutLayout L;
    L.poses = 0; L.invdepth = ba_up256(56 * nk); L.bad_obs = L.invdepth + ba_up256(8 * nl); L.chi2 = L.bad_obs + ba_up256(nr);
    L.dpos = L.chi2 + ((out_flags & 1) ? ba_up256(8 * nr) : 0);
    L.total = L.dpos + ((out_flags & 2) ? ba_up256(nr) : 0);
    return L;
}

// head of the batch's pinned block and of its device mirror, N problems: look-ahead words (one int each) | 16 int counters each |
// control blocks | device views; the result block starts at out_base, the problems' slices follow it
struct BABatchHeader { size_t flag, cnt, ctl, arr, out_base; };
static inline BABatchHeader ba_batch_header(int N, size_t sizeof_ctl, size_t sizeof_dev)
{
    const size_t n = (size_t)N;
    BABatchHeader h;
    h.flag = 0; h.cnt = ba_up256(4 * n); h.ctl = h.cnt + ba_up256(64 * n); h.arr = h.ctl + ba_up256(sizeof_ctl * n);
    h.out_base = h.arr + ba_up256(sizeof_dev * n);
    return h;
}
