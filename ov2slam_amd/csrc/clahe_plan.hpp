// clahe_plan.hpp -- host plan of the fused strip kernel's LUT computation (clahe.hip, k_clahe_apply_pyr<., true>): which of its two
// forms a geometry takes and how much dynamic LDS the work-group gets.  Plain C++ (compiled and checked by tests/test_clahe_plan.py).
//
//   tile form: one wavefront per tile, 16 lanes per tile row (clahe_lut_tiles); every wavefront owns a 32-bit histogram
//              (the strips one copy, the LUT wavefronts CH_NCOPY staggered copies);
//   row form:  the wavefront walks whole image rows, 12 bytes per lane, into the histograms of ALL tiles of the row of tiles at
//              once -- 16-bit counters, two tiles per dword, one staggered block of 256 dwords per pair of tiles.
#pragma once

#if defined(__HIPCC__)
#define OV2_CLP_HD __host__ __device__ __forceinline__
#else
#define OV2_CLP_HD static inline
#endif

#define CH_WAVE_DW 256               // dwords of a one-copy histogram
#define CH_CSTRIDE 264               // dwords between the copies of a multi-copy histogram / between the pair blocks of the row form:
                                     // bin b of copy (block) c sits in LDS bank (b + 8 c) % 64
#define CH_NCOPY 4                   // copies of the wavefronts that histogram most tiles (k_clahe_lut; the LUT wavefronts of the fused kernel)
                                     // (other copy counts: profiles/r5_clahe_histogram_variants.txt)
#define CH_MULTI_DW (CH_NCOPY * CH_CSTRIDE)
#define CH_ROW_CHUNK_DW 192          // row form: image dwords one trip of the wavefront covers (3 per lane)

// padded tile size of cv::CLAHE: the image is extended to a multiple of the tile grid (both ways as soon as one does not divide)
static inline void ov2_clahe_tile_size(int w, int h, int tiles_x, int tiles_y, int *tw, int *th)
{
    int ew = w, eh = h;
    if (!(w % tiles_x == 0 && h % tiles_y == 0)) { ew = w + (tiles_x - w % tiles_x); eh = h + (tiles_y - h % tiles_y); }
    *tw = ew / tiles_x; *th = eh / tiles_y;
}

// dynamic LDS of the fused kernel without its histograms: the packed table of a row of cells + the LUT ring of two rows of tiles
static inline long long ov2_clahe_lds_tables(int tiles_x) { return (long long)(tiles_x + 1) * 1024 + (long long)2 * tiles_x * 256; }
static inline long long ov2_clahe_lds_tile_form(int tiles_x, int nstrips, int nlut)
{
    return ov2_clahe_lds_tables(tiles_x) + ((long long)nstrips * CH_WAVE_DW + (long long)nlut * CH_MULTI_DW) * 4;
}
OV2_CLP_HD int ov2_clahe_pair_blocks(int tiles_x) { return (tiles_x + 1) / 2; }
static inline long long ov2_clahe_lds_row_form(int tiles_x) { return ov2_clahe_lds_tables(tiles_x) + (long long)ov2_clahe_pair_blocks(tiles_x) * CH_CSTRIDE * 4; }

// work-groups of `waves` wavefronts and `lds` bytes that stay resident on one CU: 160 KiB of LDS handed out in OV2_CLAHE_LDS_GRANULE
// steps, six wavefronts per SIMD at the kernel's 80 registers
#define OV2_CLAHE_LDS_GRANULE 512
static inline int ov2_clahe_resident(long long lds, int waves)
{
    const long long alloc = (lds + OV2_CLAHE_LDS_GRANULE - 1) / OV2_CLAHE_LDS_GRANULE * OV2_CLAHE_LDS_GRANULE;
    const long long by_lds = alloc > 0 ? 160 * 1024 / alloc : 24, by_waves = 24 / waves;
    return (int)(by_lds < by_waves ? by_lds : by_waves);
}

// The row form is taken when
//   * source rows and base are dword-aligned (the lanes load 12 aligned bytes);
//   * a tile's padded pixel count fits a 16-bit counter, and a lane's 12 bytes touch at most two tiles (tw >= 12);
//   * the REFLECT_101 padding right of / below the image mirrors into the last tile column / row itself (columns and rows are
//     then weighted 0, 1 or 2 -- the tile form's `tile_fast` condition and its vertical twin);
//   * one LUT wavefront does the rows of tiles;
//   * its LDS is no larger than the tile form's, or at least leaves as many work-groups resident on a CU.
static inline bool ov2_clahe_row_form(int w, int h, int tiles_x, int tiles_y, bool src_aligned, int nstrips, int nlut)
{
    int tw, th;
    ov2_clahe_tile_size(w, h, tiles_x, tiles_y, &tw, &th);
    if (!src_aligned || nlut != 1 || tw < 12 || (long long)tw * th >= 65536) return false;
    if (2 * (tiles_x - 1) * tw + tw > 2 * w - 1 || 2 * (tiles_y - 1) * th + th > 2 * h - 1) return false;
    const long long lr = ov2_clahe_lds_row_form(tiles_x), lt = ov2_clahe_lds_tile_form(tiles_x, nstrips, nlut);
    return lr <= lt || ov2_clahe_resident(lr, nstrips + nlut) >= ov2_clahe_resident(lt, nstrips + nlut);
}
static inline long long ov2_clahe_lds_fused(bool row_form, int tiles_x, int nstrips, int nlut)
{
    return row_form ? ov2_clahe_lds_row_form(tiles_x) : ov2_clahe_lds_tile_form(tiles_x, nstrips, nlut);
}
