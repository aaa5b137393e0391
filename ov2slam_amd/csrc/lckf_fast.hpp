// lckf_fast.hpp -- cv::FAST's TYPE_9_16 ring test and cornerScore<16> for one pixel of a byte tile (lckf.hip: k_lckf_fast).
// Restated from OpenCV's published fast.cpp / fast_score.cpp; the arithmetic is the one of k_fast_cells (detect.hip) and of the
// oracle's fast_corner_score.
#pragma once
#include <stdint.h>

// p: the centre pixel in a tile whose rows are PITCH bytes apart (the whole ring must lie inside the tile).  Returns the score of a
// corner (threshold .. 255: every pixel of the arc differs by more than the threshold) and 0 for a pixel that is no corner.  With
// threshold 0 a corner can score 0: it never survives the strict non-maximum suppression, so 0 is "nothing" throughout.
template <int PITCH>
__device__ __forceinline__ int lckf_fast_score(const uint8_t *p, int threshold)
{
    const int v = p[0];
    int ring[16];                           // the circle of radius 3 in cv::FAST's order (makeOffsets, patternSize 16)
    ring[0] = p[3 * PITCH];       ring[1] = p[3 * PITCH + 1];   ring[2] = p[2 * PITCH + 2];   ring[3] = p[PITCH + 3];
    ring[4] = p[3];               ring[5] = p[-PITCH + 3];      ring[6] = p[-2 * PITCH + 2];  ring[7] = p[-3 * PITCH + 1];
    ring[8] = p[-3 * PITCH];      ring[9] = p[-3 * PITCH - 1];  ring[10] = p[-2 * PITCH - 2]; ring[11] = p[-PITCH - 3];
    ring[12] = p[-3];             ring[13] = p[PITCH - 3];      ring[14] = p[2 * PITCH - 2];  ring[15] = p[3 * PITCH - 1];
    unsigned dark = 0, bright = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        dark |= (unsigned)(ring[k] < v - threshold) << k;
        bright |= (unsigned)(ring[k] > v + threshold) << k;
    }
    // 9 contiguous ring pixels: the mask doubled to 32 bits and ANDed with itself shifted by 1 .. 8
    const unsigned md = dark | (dark << 16), mb = bright | (bright << 16);
    unsigned rd = md, rb = mb;
#pragma unroll
    for (int i = 1; i <= 8; i++) { rd &= md >> i; rb &= mb >> i; }
    if (((rd | rb) & 0xFFFFu) == 0) return 0;
    // cornerScore<16>
    int d[25];
#pragma unroll
    for (int k = 0; k < 25; k++) d[k] = v - ring[k & 15];
    int a0 = threshold;
#pragma unroll
    for (int k = 0; k < 16; k += 2) {
        int a = min(d[k + 1], min(d[k + 2], d[k + 3]));
        a = min(a, min(d[k + 4], min(d[k + 5], min(d[k + 6], min(d[k + 7], d[k + 8])))));
        a0 = max(a0, min(a, d[k]));
        a0 = max(a0, min(a, d[k + 9]));
    }
    int b0 = -a0;
#pragma unroll
    for (int k = 0; k < 16; k += 2) {
        int b = max(d[k + 1], max(d[k + 2], d[k + 3]));
        b = max(b, max(d[k + 4], max(d[k + 5], max(d[k + 6], max(d[k + 7], d[k + 8])))));
        b0 = min(b0, max(b, d[k]));
        b0 = min(b0, max(b, d[k + 9]));
    }
    return -b0 - 1;
}
