// lk_plan.hpp -- the unit plan of the persistent k_fb_klt3 (lk3.hip): which (item, keypoint block) pairs of a launch hold a
// keypoint, and on which of 8 lists each waits to be pulled.  Plain C++ shared by k_lk_plan and the host (compiled and checked
// exhaustively by tests/test_lk_plan.py).
//
// A launch has `batch` items of up to nbx blocks of `kpb` keypoints; item b has n[b] of them, so only its blocks k with
// k * kpb < n[b] are units.  List r (one per XCD, see xcd_map.hpp) holds the units whose work-group id under ov2_xcd_map has
// residue r mod 8, in the order of those ids:
//   * entries j < batch / 8: ALL blocks of item 8 j + r, consecutive -- the blocks of one image pair stay on one L2 and run at
//     about the same time;
//   * entries batch / 8 + q, q < batch % 8: the left-over item b8 + q, whose ids nbx * (b8 + q) + k are dealt over the residues
//     block by block -- list r gets its blocks k = k0, k0 + 8, ... with k0 = (r - q nbx) mod 8.
// A list is therefore in ascending item order, and the 8 lists together hold every unit exactly once.
#pragma once

#if defined(__HIPCC__)
#define OV2_LKP_HD __host__ __device__ __forceinline__
#else
#define OV2_LKP_HD static inline
#endif

#define OV2_LKP_LISTS 8
// layout of the plan buffer (ints): pull counters (one 128-byte line each: they are hammered by atomics), list lengths, lists
#define OV2_LKP_CTR_STRIDE 32
#define OV2_LKP_LEN (OV2_LKP_LISTS * OV2_LKP_CTR_STRIDE)
#define OV2_LKP_UNITS (OV2_LKP_LEN + OV2_LKP_LISTS)

struct ov2_lkp_entry { int item, first, step, count; };      // units (item, first + t * step), t < count

OV2_LKP_HD int ov2_lkp_entries(int batch) { return (batch >> 3) + (batch & 7); }                // entries of every list
OV2_LKP_HD int ov2_lkp_list_cap(int batch, int nbx) { return nbx * ((batch >> 3) + 1); }         // units a list can hold
OV2_LKP_HD long long ov2_lkp_ints(int batch, int nbx) { return OV2_LKP_UNITS + (long long)OV2_LKP_LISTS * ov2_lkp_list_cap(batch, nbx); }
OV2_LKP_HD int ov2_lkp_item(int r, int j, int batch) { const int g = batch >> 3; return j < g ? 8 * j + r : 8 * g + (j - g); }
OV2_LKP_HD int ov2_lkp_blocks(int n, int nbx, int kpb) { const int nb = n > 0 ? (n - 1) / kpb + 1 : 0; return nb < nbx ? nb : nbx; }

// entry j of list r, given the keypoint count n of ITS item (ov2_lkp_item)
OV2_LKP_HD ov2_lkp_entry ov2_lkp_entry_of(int r, int j, int batch, int nbx, int kpb, int n)
{
    const int g = batch >> 3, nb = ov2_lkp_blocks(n, nbx, kpb);
    ov2_lkp_entry e;
    if (j < g) { e.item = 8 * j + r; e.first = 0; e.step = 1; e.count = nb; }
    else {
        const int q = j - g;
        e.item = 8 * g + q;
        e.first = (r - q * nbx) & 7;
        e.step = 8;
        e.count = e.first < nb ? (nb - e.first + 7) >> 3 : 0;
    }
    return e;
}

// a unit as one int, and back
OV2_LKP_HD int ov2_lkp_pack(int item, int block, int nbx) { return item * nbx + block; }
OV2_LKP_HD void ov2_lkp_unpack(int unit, int nbx, int *item, int *block) { *item = unit / nbx; *block = unit - *item * nbx; }

// List r written entry by entry (what k_lk_plan does with one thread per entry and a prefix sum over the counts): returns its
// length.  n == nullptr: n_all keypoints in every item.
OV2_LKP_HD int ov2_lkp_fill_list(int r, const int *n, int n_all, int batch, int nbx, int kpb, int *list)
{
    int len = 0;
    for (int j = 0; j < ov2_lkp_entries(batch); j++) {
        const int item = ov2_lkp_item(r, j, batch);
        const ov2_lkp_entry e = ov2_lkp_entry_of(r, j, batch, nbx, kpb, n ? n[item] : n_all);
        for (int t = 0; t < e.count; t++) list[len++] = ov2_lkp_pack(e.item, e.first + t * e.step, nbx);
    }
    return len;
}
