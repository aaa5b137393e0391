// fivept_dev.hpp -- the relative-pose search of fivept.hip (k_e5_solve, k_e5_score, k_e5_pick) as one host step on buffers the caller
// owns, so that another driver (epifilter.hip: epipolar2d2dFiltering) can put the search between its own kernels on one stream
// without a synchronisation.  ov2_epipolar_ransac_batch is this step around one upload, one download and one synchronisation.  The
// kernels themselves stay in fivept.hip (the pattern of p3p_dev.hpp): one code object holds them, whoever enqueues.
#pragma once
#include "common.hpp"

struct E5Item { int n, S, pt0, row0; };                // points, sample rows, and where both start in the call's arrays
struct E5Out { double model[12]; double score; int best_row, iterations, rows_consumed, status, n_inliers, n_outliers; };
static_assert(sizeof(E5Out) == 128, "E5Out layout");

// device pointers.  Inputs: items (one per problem; may be written by a kernel earlier on the stream), bv1 / bv2 (3 doubles per
// point), samples (two int4 per row).  Own: models (12 doubles per row), valid (1), score (8).  Results: out (one per problem),
// outliers (ascending, problem b's at its pt0).
struct E5Args {
    const E5Item *items; const double *bv1; const double *bv2; const int4 *samples;
    double *models; uint8_t *valid; double *score;
    E5Out *out; int *outliers;
    int max_iterations; double threshold, probability;
};

// draw j of the sample stream (ov2_p3p_draw_samples, ov2_epipolar_draw_samples): splitmix64 of seed + (j + 1) * the golden gamma
__host__ __device__ static inline unsigned long long e5_splitmix64(unsigned long long seed, unsigned long long j)
{
    unsigned long long z = seed + (j + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The three launches over problems [0, n_items): s_max bounds every problem's S (the grids follow it, each kernel takes the real
// counts from the E5Item it reads; with s_max == 0 only k_e5_pick runs).  No synchronisation.
int e5_enqueue(hipStream_t s, const E5Args &a, int n_items, int s_max);
