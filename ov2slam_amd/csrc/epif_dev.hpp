// epif_dev.hpp -- epipolar2d2dFiltering's chain (epifilter.hip: k_epif_gather, the search of fivept_dev.hpp, k_epif_decide) as host
// steps on a device block the caller owns, so that the lock-step tracker can later put it between k_pose_select and k_pose_pack on
// one stream without a host round trip.  ov2_epipolar_filter_batch is the same launches around one upload, one download and one
// synchronisation, on a block packed to the items' real sizes.
#pragma once
#include "common.hpp"
#include "fivept_dev.hpp"

// 208 bytes.  cur0 / kf0 / row0: where the item's keypoint slots, keyframe slots and sample rows start in the block's arrays (the
// chain's own per-match arrays use the current frame's slots: a frame has at most n_cur matches)
struct EpifItem {
    int cur0, n_cur, kf0, n_kf;
    int row0, n_rows, nb3dkps, nbkfs;
    unsigned long long seed;
    double cur_Twc[7], kf_Tcw[7], kf_Twc[7];
};
static_assert(sizeof(EpifItem) == 208, "EpifItem layout");
struct EpifOut {
    double model[12], F[9], Twc_model[7], score;
    float parallax;
    int action, m, epifrom3dkps, do_optimize, nb3dkps, status, best_row, iterations, rows_consumed, n_inliers, n_outliers;
    int n_removed_ransac, n_removed_sampson, pose_from_model, searched, pad[2];
};
static_assert(sizeof(EpifOut) == 304, "EpifOut layout");

// Offsets from the block's base, every section 16-byte aligned.  [0, o_up): the chain's INPUTS (items, cur_lmid 4, cur_unpx 8,
// cur_bv 24, cur_is3d 1 per current slot; kf_lmid 4, kf_unpx 8, kf_bv 24 per keyframe slot).  [o_up, o_down): its own (bv1 24, bv2 24,
// outliers 4 per current slot; E5Item, E5Out per item; models 96, valid 1, score 8 per row).  [o_down, total): its RESULTS (EpifOut
// per item; removed 1, pair_cur 4, err 4 per current slot; samples 32 per row).
struct EpifLayout {
    size_t B, NC, NK, NR;        // items, current slots, keyframe slots, sample rows
    int s_max;                   // the largest n_rows
    size_t o_it, o_lm, o_un, o_bv, o_3d, o_kl, o_ku, o_kb, o_up;
    size_t o_b1, o_b2, o_ol, o_e5, o_eo, o_md, o_va, o_sc, o_down;
    size_t o_out, o_rm, o_pc, o_er, o_sm, total;
};

// the layout of a block with NC / NK / NR slots in all (the packed form: the sums over the items)
void epif_layout(size_t n_items, size_t NC, size_t NK, size_t NR, int s_max, EpifLayout *L);
// The CAPACITY form, for a block whose items are written on the device: item b owns n_max current and keyframe slots at b * n_max and
// n_rows rows at b * n_rows.  OV2_EINVAL beyond the capacity of ov2_epipolar_filter_batch.
int epif_layout_capacity(int n_items, int n_max, int n_rows, EpifLayout *L);
// what ov2_epipolar_filter_batch checks in its params
int epif_check_params(const ov2_epifilter_params *params);
// The chain on items [0, n_items) of the block `ds`: the gather (join, parallax, gate, packed bearings, E5Item, sample table), the
// three launches of the search, the decision.  No synchronisation; the results are left at [o_down, total).
int epif_chain_enqueue(hipStream_t s, const ov2_epifilter_params *params, const EpifLayout &L, uint8_t *ds, int n_items);

// ---- device: what the two gather kernels share (k_epif_gather here, k_minit_gather in monoinit.hip) ----------------------------------
#pragma clang fp contract(off)

#define EPIF_THREADS 256               // four wavefronts per item
#define EPIF_WIN 2048                  // stream positions per window of the draw (8.5 KB of LDS)

__device__ __forceinline__ int epif_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the row that starts at position p of the window v[0, W): its eight distinct values and the draws it consumed, 0 when the window
// ends before the row is full
__device__ __forceinline__ int epif_row_walk(const unsigned short *v, int p, int W, int (&row)[8])
{
    int k = 0, c = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) row[q] = -1;
    while (k < 8 && p + c < W) {
        const int x = v[p + c];
        c++;
        bool dup = false;
#pragma unroll
        for (int q = 0; q < 8; q++) dup = dup || row[q] == x;      // empty slots hold -1
        if (dup) continue;
#pragma unroll
        for (int q = 0; q < 8; q++) row[q] = q == k ? x : row[q];
        k++;
    }
    return k == 8 ? c : 0;
}

// The table of ov2_epipolar_draw_samples(seed, m, S) into tab (two int4 per row), by the EPIF_THREADS lanes of one work-group (t: the
// lane's index in it; every lane calls, m >= 8 and S >= 1 are uniform).  Draw j is splitmix64(seed, j) % m; a slot that repeats an
// earlier slot of its row is drawn again.  A row always starts from an empty state, so "the row that starts at stream position p
// consumes cnt(p) draws" is a function of p alone: a window of the stream is evaluated for every p by lanes, the row starts are then the
// chain 0, cnt(0), cnt(0) + cnt(cnt(0)), ... (dependent LDS reads, eight rows per read), and the rows are filled by lanes again.
// LDS, all of it the caller's and free for the taking once the work-group has passed a barrier behind its last use: s_a (2 EPIF_WIN
// unsigned shorts: the window and its counts), s_c (3 EPIF_WIN: the counts over 2, 4 and 8 rows), s_start (EPIF_WIN / 8).
__device__ __forceinline__ void epif_draw_table(unsigned long long seed, int m, int S, int4 *tab, unsigned short *s_a, unsigned short *s_c,
                                                unsigned short *s_start, int t)
{
    unsigned short *s_v = s_a, *s_cnt = s_v + EPIF_WIN;
    const unsigned um = (unsigned)m, c32 = (0xffffffffu % um + 1u) % um;       // 2^32 mod m
    int r = 0;
    unsigned long long j0 = 0;
    bool whole = false;                                            // the last window was a short one and held no whole row
    for (int win = 0; win <= 2 * S && r < S; win++) {              // a window completes a row, or is evaluated again as a whole one, or ends the loop
        int W = 16 * (S - r) + 64;                                 // a few rows left need no whole window: an estimate, not a bound
        W = (whole || W > EPIF_WIN) ? EPIF_WIN : W;
        for (int p = t; p < W; p += EPIF_THREADS) {                // z % m through 32-bit halves: m < 2^11, so nothing overflows
            const unsigned long long z = e5_splitmix64(seed, j0 + (unsigned long long)p);
            const unsigned hi = (unsigned)(z >> 32), lo = (unsigned)z;
            s_v[p] = (unsigned short)(((hi % um) * c32 + lo % um) % um);
        }
        __syncthreads();
        for (int p = t; p < W; p += EPIF_THREADS) {
            int row[8];
            s_cnt[p] = (unsigned short)epif_row_walk(s_v, p, W, row);
        }
        __syncthreads();
        // the counts over 2, 4 and 8 consecutive rows (0 where one of them runs past the window), so that the chain below makes
        // one dependent read per EIGHT rows
        for (int lv = 0; lv < 3; lv++) {
            const unsigned short *src = lv == 0 ? s_cnt : s_c + (lv - 1) * EPIF_WIN;
            unsigned short *dst = s_c + lv * EPIF_WIN;
            for (int p = t; p < W; p += EPIF_THREADS) {
                const int c = src[p], q = p + c;
                const int c2 = (c != 0 && q < W) ? src[q] : 0;
                dst[p] = (unsigned short)(c2 != 0 ? c + c2 : 0);
            }
            __syncthreads();
        }
        const unsigned short *s_c8 = s_c + 2 * EPIF_WIN;
        int ng = 0, pos = 0;                                       // uniform: every lane reads the same words
        while (pos < W && r + 8 * (ng + 1) <= S) {
            const int c = s_c8[pos];
            if (c == 0) break;                                     // fewer than eight whole rows are left in the window
            if (t == 0) s_start[ng] = (unsigned short)pos;
            ng++; pos += c;
        }
        if (t == 0) s_start[ng] = (unsigned short)pos;             // the tail: up to seven rows, one read each
        int nt = 0;
        while (pos < W && r + 8 * ng + nt < S && nt < 8) {
            const int c = s_cnt[pos];
            if (c == 0) break;                                     // the row runs past the window
            nt++; pos += c;
        }
        const int nr = 8 * ng + nt;
        __syncthreads();
        if (nr == 0) {
            if (W == EPIF_WIN) break;                              // a row of more than EPIF_WIN draws: see the header
            whole = true;                                          // the short window was the estimate's fault: the same positions again,
            continue;                                              // as a whole window (the barrier above covers the rewrite of s_v)
        }
        whole = false;
        for (int q = t; q < nr; q += EPIF_THREADS) {
            int row[8], p = s_start[q >> 3];
            for (int k = 0; k < (q & 7); k++) p += s_cnt[p];
            epif_row_walk(s_v, p, W, row);
            tab[2 * (r + q)] = make_int4(row[0], row[1], row[2], row[3]);
            tab[2 * (r + q) + 1] = make_int4(row[4], row[5], row[6], row[7]);
        }
        r += nr; j0 += (unsigned long long)pos;
        __syncthreads();                                           // s_v and s_start are rewritten by the next window
    }
    for (int rr = r + t; rr < S; rr += EPIF_THREADS) {             // the bound was met: rows the search skips
        tab[2 * rr] = make_int4(-1, -1, -1, -1);
        tab[2 * rr + 1] = make_int4(-1, -1, -1, -1);
    }
}
