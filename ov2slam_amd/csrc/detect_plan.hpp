// detect_plan.hpp -- the ONE place that knows the host decisions of the grid detectors (detect.hip): the size constants, the strip
// kernel's packing and LDS bytes, which k_grid_select instance and how much LDS a selection takes, the scratch layouts, the
// reference's adaptation rules and the geometry an entry point accepts.  Plain C++ (no HIP types, no context): detect.hip
// includes it ahead of the kernels, tests/test_detect_plan.py compiles it alone with g++.
#pragma once
#include <stddef.h>
#include "stage.hpp"

#define DET_MAX_CELL 64
#define DET_CHUNK 1024     // images per pass of the batch entry points (the response maps of a pass live in the scratch: 1.3 MB per EuRoC image)
#define DET_SORT_CAP 512        // corners of a cell that can enter the emulated sort (non-adjacent after NMS: <= 32 x 32 / 2 for cs = 64, halved again by N3)
#define STRIP_MAX_CELLS 8
#define DET_SEL_THREADS_BATCH 512
#define DET_LDS_BYTES ((size_t)160 * 1024)                  // LDS of a gfx950 work-group, static + dynamic
#define DET_SELECT_STATIC_LDS 256                           // bound on k_grid_select's static LDS (locks, counters); tests/test_detect_cases.py holds the build to it
#define DET_CAND_BYTES 16                                   // sizeof(CellCand), sizeof(SelectOut): detect.hip asserts both
#define DET_SELECT_OUT_BYTES 56

// ---------------------------------------------------------------------------------- k_mineig_strip
// dynamic LDS of k wavefronts: the blurred bytes of their 64 k columns, and the staged map columns (row pitch 65 floats)
static inline size_t det_strip_lds(int cell, int k) { return (((size_t)cell * 64 * k + 15) & ~(size_t)15) + (size_t)k * cell * 65 * 4; }

struct DetStrip { int cells, waves, owned; size_t lds; };    // cells per work-group (0: nothing fits), wavefronts, owned columns per wavefront

// The cells per group / wavefronts per group that leave the fewest lanes idle: a wavefront owns at most 60 of its 64 columns.  Only
// what fits the LDS beside the kernel's static `static_lds` bytes is a choice: at cell 64 the densest packing (7 cells on 8
// wavefronts) needs 165888 bytes, so (6, 7) runs
static inline DetStrip det_strip_geometry(int cell, int static_lds)
{
    DetStrip g = {0, 0, 0, 0};
    double best_e = 0.0;
    for (int nc = 1; nc <= STRIP_MAX_CELLS; nc++) {
        const int k = (nc * cell + 59) / 60;
        if (k > 8) break;
        if (det_strip_lds(cell, k) + (size_t)static_lds > DET_LDS_BYTES) continue;
        const double e = (double)nc * cell / (64.0 * k);
        if (g.cells == 0 || e > best_e + 1e-9) { best_e = e; g.cells = nc; g.waves = k; }
    }
    if (g.cells) { g.owned = (g.cells * cell + g.waves - 1) / g.waves; g.lds = det_strip_lds(cell, g.waves); }
    return g;
}

// det_strip: OV2_OPT_DETECT_STRIP (-1 auto: batches, 0 one wavefront per cell, 1 the strip kernel)
static inline bool det_use_strip(int det_strip, int ncells, int items) { return det_strip == 1 || (det_strip < 0 && (long long)ncells * items >= 2048); }

// ---------------------------------------------------------------------------------- k_grid_select
// Dynamic LDS: exclusion mask + cell tables (+ the sort areas of the libstdc++ tie order, FAST only).
// *slots = sort areas that fit (<= 16); returns 0 when the image does not fit at all.
static inline size_t det_select_lds(int w, int h, int cell, int mode, bool libstdcxx_tie, int *slots)
{
    const int nw = w / cell, nh = h / cell, ncells = nw * nh, wpr = (w + 31) / 32;
    const size_t base = (size_t)h * wpr * 4 + 64 * 4 + (size_t)ncells * 16 + (size_t)nh * 4 + (((size_t)(nh + 1) * (nw + 1) + 3) & ~(size_t)3) + (size_t)ncells * 8;
    const size_t limit = DET_LDS_BYTES - DET_SELECT_STATIC_LDS;
    *slots = 0;
    if (base > limit) return 0;
    if (mode != 0 || !libstdcxx_tie) return base;
    const size_t area = (size_t)(DET_SORT_CAP + 72) * 4;
    const size_t fit = (limit - base) / area;
    if (fit == 0) return 0;
    *slots = fit > 16 ? 16 : (int)fit;
    return base + (size_t)*slots * area;
}

// the instances' (MAXROW, CHUNKS): (36,1) and (52,1) cover the reference cell sizes with compile-time column indices, (32,2) the rest
constexpr struct DetSelectClass { int maxrow, chunks; } DET_SELECT_CLASS[3] = {{36, 1}, {52, 1}, {32, 2}};
static inline int det_select_class(int cell) { return cell <= 36 ? 0 : (cell <= 52 ? 1 : 2); }
// One image: sixteen wavefronts, a row of cells each (latency).  Batches: EIGHT (rows w, w + 8 -- the anti-diagonal dependence keeps
// at most nwcells / 2 rows busy at a time anyway), so that two work-groups share a CU's sixteen wavefront slots (106 VGPRs: four
// per SIMD) instead of one
static inline int det_select_threads(int items) { return items >= 64 ? DET_SEL_THREADS_BATCH : 1024; }
// capacity of an image's output list: a point per cell for FAST, primaries and secondaries for single scale
static inline int det_out_cap(int mode, int ncells) { return mode == 0 ? ncells : 2 * ncells; }

// ---------------------------------------------------------------------------------- scratch layouts (byte offsets)
static inline size_t det_map_bytes(int cell, int ncells, int mode) { return (size_t)ncells * cell * cell * (mode == 0 ? 1 : 4); }

// one image: [img w*h (upload only)][maps][cur 8*ncur][out 8*2*ncells][SelectOut][candidates][free-cell list (k_free_cells)]
struct DetScratch { size_t img, map, cur, out, so, cand, free_list, total; };
static inline DetScratch det_scratch(int w, int h, int cell, int mode, int ncur, bool upload)
{
    const int ncells = (w / cell) * (h / cell);
    const size_t map = upload ? up256((size_t)w * h) : 0, cur = up256(map + det_map_bytes(cell, ncells, mode));
    const size_t out = up256(cur + 8 * (size_t)(ncur > 0 ? ncur : 1)), so = out + 16 * (size_t)ncells;       // (the counters right behind the points: one copy back)
    const size_t cand = up256(so + DET_SELECT_OUT_BYTES), free_list = cand + DET_CAND_BYTES * (size_t)ncells;
    return {0, map, cur, out, so, cand, free_list, free_list + 4 * ((size_t)ncells + 1)};
}

// A batch: passes of `chunk` images share a scratch set [maps][candidates][free-cell lists] (map, cand, free_list: offsets in a
// set), then every item's SelectOut and its threshold / quality.  More than one pass: TWO sets of half a chunk, the passes
// alternating between the context's stream and an auxiliary one -- the selection sweep of a pass (a dependency chain: two work-groups
// per CU, the vector units nearly idle) then runs beside the response kernel of the next pass (issue-bound) instead of between two of them
struct DetBatchScratch { int sets, chunk; size_t map, cand, free_list, set_bytes, so, par, total; };
static inline DetBatchScratch det_batch_scratch(int cell, int ncells, int mode, int items)
{
    const int sets = items > DET_CHUNK / 2 ? 2 : 1, chunk = sets == 2 ? DET_CHUNK / 2 : items;
    const size_t cand = up256((size_t)chunk * det_map_bytes(cell, ncells, mode)), free_list = cand + (size_t)chunk * ncells * DET_CAND_BYTES;
    const size_t set_bytes = up256(free_list + (size_t)chunk * 4 * ((size_t)ncells + 1)), so = (size_t)sets * set_bytes;
    const size_t par = up256(so + (size_t)items * DET_SELECT_OUT_BYTES);
    return {sets, chunk, 0, cand, free_list, set_bytes, so, par, par + (size_t)items * 8};
}

// ---------------------------------------------------------------------------------- the reference's adaptation rules
// FAST threshold after a call (feature_extractor.cpp:546-552), int *= double truncates
static inline int det_adapt_fast_th(int th, int nbkps, int nbempty)
{
    if ((double)nbkps < 0.5 * (double)nbempty && nbempty > 10) return (int)(th * 0.66);
    return nbkps == nbempty ? (int)(th * 1.5) : th;
}
// quality after a call (:418-423; n is the size after the secondary top-up)
static inline double det_adapt_quality(double q, int n, int ncells, int nboccup)
{
    if ((double)n < 0.33 * (double)(ncells - nboccup)) return q / 2.;
    return (double)n > 0.9 * (double)(ncells - nboccup) ? q * 1.5 : q;
}

// ---------------------------------------------------------------------------------- what an entry point accepts
enum DetCheck { DET_CHECK_OK = 0, DET_CHECK_CELL, DET_CHECK_SIZE, DET_CHECK_MASK_LDS };
static inline DetCheck det_check_geometry(int w, int h, int cell, int mode, bool libstdcxx_tie)
{
    if (cell < 8 || cell > DET_MAX_CELL) return DET_CHECK_CELL;
    if (w >= 65536 || h >= 32768) return DET_CHECK_SIZE;
    int slots;
    return (w / cell) * (h / cell) > 0 && det_select_lds(w, h, cell, mode, libstdcxx_tie, &slots) == 0 ? DET_CHECK_MASK_LDS : DET_CHECK_OK;    // (no cell: an empty result)
}
