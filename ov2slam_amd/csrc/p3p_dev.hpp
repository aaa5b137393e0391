// p3p_dev.hpp -- the absolute-pose search of p3p.hip as three host steps on buffers the caller owns, so that another driver
// (pnp.hip: computePose) can put the search in front of its own kernels on one stream without a synchronisation in between.
// ov2_p3p_ransac_batch is these steps around one upload, one download and one synchronisation.
#pragma once
#include "common.hpp"

struct P3Item { int n, S, pt0, row0; };
struct P3Out { double model[12]; double score; int best_row, iterations, rows_consumed, status, n_inliers, n_outliers; };
static_assert(sizeof(P3Out) == 128, "P3Out layout");

// One staging block, every section 16-byte aligned: [items 16 B][bv 24][X 24][samples 16] go up, [out 128][outliers 4][valid 1]
// [score 8] come down (the last two only for a trace), [models 96] stays on the device.  Offsets are from the block's base.
struct P3Plan {
    size_t B, NP, NR;            // problems, points and sample rows of the call
    int n_max, s_max;            // the largest problem / sample table
    bool trace;
    size_t o_it, o_bv, o_X, o_sm, o_out, o_ol, o_va, o_sc, o_md, total;
};

// the checks of ov2_p3p_ransac_batch on params and problems (results may be NULL: then no result buffer is looked at), and the plan
int p3p_plan(const ov2_p3p_params *params, int n_items, const ov2_p3p_problem *problems, const ov2_p3p_result *results, P3Plan *plan);
// The plan in its capacity form, for a block whose items are written on the device: problem b owns n_max points at b * n_max and
// n_rows rows at b * n_rows.  The grids and the LDS size of p3p_enqueue follow these bounds; every kernel takes the real counts from
// the P3Item it reads (a problem's bits do not depend on the bounds: the LDS path is chosen by its own n).  No trace.  OV2_EINVAL
// beyond the capacity of ov2_p3p_ransac_batch.
int p3p_plan_capacity(int n_items, int n_max, int n_rows, P3Plan *plan);
// fills [0, o_out) of the host block
void p3p_stage(const P3Plan &pl, const ov2_p3p_problem *problems, uint8_t *hs);
// the three launches on the device block (whose [0, o_out) holds what p3p_stage wrote); results stay in HBM: P3Out per problem at
// o_out, the ascending outlier lists at o_ol (problem b's at its point offset)
int p3p_enqueue(hipStream_t s, const ov2_p3p_params *params, const P3Plan &pl, uint8_t *ds);
