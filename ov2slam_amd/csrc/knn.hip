// knn.hip -- the loop closer's descriptor matching for gfx950 (the reference's LoopCloser::knnMatching, src/loop_closer.cpp:378-459:
// cv::BFMatcher(cv::NORM_HAMMING).knnMatch(query, train, vmatches, 2), then the distance gate and the ratio test of :432-449):
//   k_knn          ONE LANE PER QUERY ROW, its 32 bytes in 8 VGPRs.  A work-group of KNN_QUERIES lanes stages the item's train rows
//                  into LDS KNN_TILE rows at a time (16-byte global loads, consecutive lanes on consecutive 16 bytes), then every
//                  lane walks the tile: all lanes read the same LDS row, so the two 16-byte reads per row are broadcasts without
//                  bank conflicts.  Per row 8 xor + popcount and the top-2 update with strict `<`, rows in ascending order: that is
//                  the lexicographic (distance, train row) order of OpenCV's batchDistance with no atomics and no reduction, so
//                  two runs give the same bytes.  grid.x = query tiles, grid.y = item, grid.z = ranges of train tiles.
//   k_knn_merge    only when grid.z > 1 (a call with too few work-groups to give every CU one, and more than one train tile): one
//                  lane per query row inserts the ranges' two candidates each, ranges in ascending order, with the same strict
//                  insertion -- the order-free definition (the two smallest (distance, train row) pairs) makes the split legal.
// Integers throughout except the ratio test, (double)d0 <= (double)d1 * ratio, one fp64 product per query row.
// tests/knn_ref.py is the same arithmetic in numpy.  The pairs (query row, train row) of the good rows are compacted on the host
// after the one download: they come in query order, as the reference appends them.
#include "common.hpp"
#include <climits>
#include <cmath>

#pragma clang fp contract(off)

constexpr int KNN_QUERIES = 256;   // query rows (lanes) per work-group
constexpr int KNN_TILE = 256;      // train rows per LDS tile: 8 KB
constexpr int KNN_AHEAD = 4;       // train rows whose LDS reads are issued together
constexpr int KNN_FILL = 256;      // work-groups that give every CU of the device one: below that the train tiles are split over grid.z

// One batch item.  Query and train rows are concatenated over the batch; q0 / t0 are the item's first rows.
struct KnItem { int n_q, n_t, q0, t0; };

struct KnArgs {
    const KnItem *items;
    const uint4 *query; const uint4 *train;     // two uint4 per row
    int2 *idx; int2 *dist; uint8_t *good;
    int max_dist; double ratio;
    int chunk_tiles;                            // train tiles per grid.z range
    int nq_total;                               // query rows of the call
    int4 *part;                                 // grid.z > 1: (d0, i0, d1, i1) per (range, query row)
};

__device__ __forceinline__ int kn_hamming(uint4 qa, uint4 qb, uint4 ta, uint4 tb)
{
    return __popc(qa.x ^ ta.x) + __popc(qa.y ^ ta.y) + __popc(qa.z ^ ta.z) + __popc(qa.w ^ ta.w) +
           __popc(qb.x ^ tb.x) + __popc(qb.y ^ tb.y) + __popc(qb.z ^ tb.z) + __popc(qb.w ^ tb.w);
}
// batchDistance's insertion for K = 2.  Both comparisons are strict: among equal distances the row met first (the lower one) stays in front.
__device__ __forceinline__ void kn_insert(int d, int row, int &d0, int &d1, int &i0, int &i1)
{
    if (d < d1) {
        const bool first = d < d0;
        d1 = first ? d0 : d;  i1 = first ? i0 : row;
        d0 = first ? d : d0;  i0 = first ? row : i0;
    }
}

// :432-449.  No neighbour at all (an empty train set): the reference returns before it matches, nothing is good.
__device__ __forceinline__ void kn_finish(const KnArgs &a, size_t o, int d0, int d1, int i0, int i1)
{
    const bool good = i0 >= 0 && (i1 < 0 || (d0 <= a.max_dist && (double)d0 <= (double)d1 * a.ratio));
    a.idx[o] = make_int2(i0, i1);
    a.dist[o] = make_int2(i0 >= 0 ? d0 : -1, i1 >= 0 ? d1 : -1);
    a.good[o] = good ? 1 : 0;
}

__global__ __launch_bounds__(KNN_QUERIES) void k_knn(KnArgs a)
{
    __shared__ uint4 tile[2 * KNN_TILE];
    const KnItem it = a.items[blockIdx.y];
    if ((int)blockIdx.x * KNN_QUERIES >= it.n_q) return;              // the whole work-group: no barrier is left behind
    const int q = (int)blockIdx.x * KNN_QUERIES + (int)threadIdx.x;
    const bool live = q < it.n_q;
    const bool wave_live = q - (int)(threadIdx.x & 63) < it.n_q;      // a wavefront past the last query row only helps to stage
    uint4 qa = make_uint4(0, 0, 0, 0), qb = qa;
    if (live) {
        qa = a.query[2 * ((size_t)it.q0 + q)];
        qb = a.query[2 * ((size_t)it.q0 + q) + 1];
    }
    int d0 = INT_MAX, d1 = INT_MAX, i0 = -1, i1 = -1;                 // batchDistance, K = 2
    const uint4 *tr = a.train + 2 * (size_t)it.t0;
    const int ntiles = it.n_t > 0 ? (it.n_t - 1) / KNN_TILE + 1 : 0;
    const int t_lo = (int)blockIdx.z * a.chunk_tiles;
    const int t_hi = ntiles - t_lo < a.chunk_tiles ? ntiles : t_lo + a.chunk_tiles;
    for (int t = t_lo; t < t_hi; t++) {
        const int r0 = t * KNN_TILE;
        const int rows = it.n_t - r0 < KNN_TILE ? it.n_t - r0 : KNN_TILE;
        __syncthreads();                                              // the previous tile has been read
        for (int v = (int)threadIdx.x; v < 2 * rows; v += KNN_QUERIES) tile[v] = tr[2 * (size_t)r0 + v];
        __syncthreads();
        if (!wave_live) continue;
        int r = 0;
        for (; r + KNN_AHEAD <= rows; r += KNN_AHEAD) {               // the LDS reads of KNN_AHEAD rows are in flight before the first is used
            uint4 ta[KNN_AHEAD], tb[KNN_AHEAD];
#pragma unroll
            for (int j = 0; j < KNN_AHEAD; j++) { ta[j] = tile[2 * (r + j)]; tb[j] = tile[2 * (r + j) + 1]; }
#pragma unroll
            for (int j = 0; j < KNN_AHEAD; j++) kn_insert(kn_hamming(qa, qb, ta[j], tb[j]), r0 + r + j, d0, d1, i0, i1);
        }
        for (; r < rows; r++) kn_insert(kn_hamming(qa, qb, tile[2 * r], tile[2 * r + 1]), r0 + r, d0, d1, i0, i1);
    }
    if (!live) return;
    const size_t o = (size_t)it.q0 + q;
    if (gridDim.z == 1) kn_finish(a, o, d0, d1, i0, i1);
    else a.part[(size_t)blockIdx.z * (size_t)a.nq_total + o] = make_int4(d0, i0, d1, i1);     // a range past the item's last tile: (INT_MAX, -1) twice
}

// splits > 1: the ranges' candidates in ascending range order.  An unset candidate is (INT_MAX, -1), which the strict insertion ignores.
__global__ __launch_bounds__(256) void k_knn_merge(KnArgs a, int splits)
{
    const int o = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (o >= a.nq_total) return;
    int d0 = INT_MAX, d1 = INT_MAX, i0 = -1, i1 = -1;
    for (int z = 0; z < splits; z++) {
        const int4 p = a.part[(size_t)z * (size_t)a.nq_total + o];
        kn_insert(p.x, p.y, d0, d1, i0, i1);
        kn_insert(p.z, p.w, d0, d1, i0, i1);
    }
    kn_finish(a, (size_t)o, d0, d1, i0, i1);
}

int ov2_knn_match_batch(ov2_ctx *ctx, const ov2_knn_params *params, int n_items, const ov2_knn_item *items, ov2_knn_result *results)
{
    // the inputs first, the context last: a malformed input is reported without a device
    OV2_REQUIRE(params, OV2_EINVAL, "NULL params");
    OV2_REQUIRE(n_items >= 0, OV2_EINVAL, "n_items < 0");
    OV2_REQUIRE(n_items == 0 || (items && results), OV2_EINVAL, "NULL item / result array");
    OV2_REQUIRE(n_items <= 65535, OV2_EUNSUPPORTED, "more than 65535 items in one call");
    OV2_REQUIRE(params->desc_bytes == 32, OV2_EUNSUPPORTED, "descriptors of 32 bytes only");
    OV2_REQUIRE(params->max_dist >= 0, OV2_EINVAL, "max_dist < 0");
    OV2_REQUIRE(std::isfinite(params->ratio) && params->ratio >= 0., OV2_EINVAL, "ratio negative or not finite");
    size_t NQ = 0, NT = 0;
    int q_max = 0, t_max = 0;
    for (int b = 0; b < n_items; b++) {
        const ov2_knn_item &k = items[b];
        const ov2_knn_result &r = results[b];
        OV2_REQUIRE(k.n_query >= 0 && k.n_train >= 0, OV2_EINVAL, "negative count (n_query / n_train)");
        OV2_REQUIRE(k.n_query == 0 || k.query, OV2_EINVAL, "query == NULL");
        OV2_REQUIRE(k.n_train == 0 || k.train, OV2_EINVAL, "train == NULL");
        OV2_REQUIRE(k.n_query == 0 || (r.idx && r.dist && r.good && r.pair_query && r.pair_train), OV2_EINVAL,
                    "NULL result buffer (idx / dist / good / pair_query / pair_train)");
        NQ += (size_t)k.n_query; NT += (size_t)k.n_train;
        q_max = k.n_query > q_max ? k.n_query : q_max;
        t_max = k.n_train > t_max ? k.n_train : t_max;
    }
    OV2_REQUIRE(NQ <= 0x7fffffff && NT <= 0x7fffffff, OV2_EUNSUPPORTED, "more than 2^31 - 1 query or train rows in one call");
    OV2_REQUIRE(ctx, OV2_EINVAL, "NULL context");
    if (n_items == 0) return OV2_OK;

    // staging: [items 16 B][query 32][train 32], then the outputs [idx 8][dist 8][good 1]; every section 16-byte aligned.  On the
    // device only, behind them: the ranges' candidates [part 16 per range and query row] when the train tiles are split
    const size_t B = (size_t)n_items;
    StageCursor c(16);
    const size_t o_it = c.take(sizeof(KnItem) * B), o_q = c.take(32 * NQ), o_t = c.take(32 * NT);
    const size_t o_out = c.take(8 * NQ), o_d = c.take(8 * NQ), o_g = c.take(NQ), total = c.off;
    // Few work-groups and several train tiles: ranges of tiles over grid.z, so that a single call is not one wavefront's walk
    // over all train rows.  A call that fills the device anyway keeps the whole walk in one work-group and needs no merge.
    const int q_tiles = (q_max + KNN_QUERIES - 1) / KNN_QUERIES, t_tiles = t_max > 0 ? (t_max - 1) / KNN_TILE + 1 : 0;
    const long long wgs = (long long)q_tiles * n_items;
    int splits = 1, chunk_tiles = t_tiles > 0 ? t_tiles : 1;
    if (t_tiles > 1 && wgs > 0 && KNN_FILL / wgs > 1) {
        const int want = (int)(KNN_FILL / wgs) < t_tiles ? (int)(KNN_FILL / wgs) : t_tiles;
        chunk_tiles = (t_tiles + want - 1) / want;
        splits = (t_tiles + chunk_tiles - 1) / chunk_tiles;
    }
    const size_t part_bytes = splits > 1 ? 16 * NQ * (size_t)splits : 0;      // device only, behind the outputs
    Stage st;
    int rc = st.open(ctx, total + part_bytes, total);  if (rc) return rc;
    uint8_t *hs = st.h, *ds = st.d;
    size_t q0 = 0, t0 = 0;
    for (int b = 0; b < n_items; b++) {
        const ov2_knn_item &k = items[b];
        const KnItem it{k.n_query, k.n_train, (int)q0, (int)t0};
        memcpy(hs + o_it + sizeof(KnItem) * b, &it, sizeof(KnItem));
        if (k.n_query) memcpy(hs + o_q + 32 * q0, k.query, 32 * (size_t)k.n_query);
        if (k.n_train) memcpy(hs + o_t + 32 * t0, k.train, 32 * (size_t)k.n_train);
        q0 += (size_t)k.n_query; t0 += (size_t)k.n_train;
    }
    if (NQ > 0) {
        rc = st.upload(0, o_out);  if (rc) return rc;
        KnArgs a;
        a.items = (const KnItem *)(ds + o_it);
        a.query = (const uint4 *)(ds + o_q); a.train = (const uint4 *)(ds + o_t);
        a.idx = (int2 *)(ds + o_out); a.dist = (int2 *)(ds + o_d); a.good = ds + o_g;
        a.max_dist = params->max_dist; a.ratio = params->ratio;
        a.chunk_tiles = chunk_tiles; a.nq_total = (int)NQ; a.part = (int4 *)(ds + total);
        hipLaunchKernelGGL(k_knn, dim3(q_tiles, n_items, splits), dim3(KNN_QUERIES), 0, ctx->stream, a);
        OV2_HIP_CHECK(hipGetLastError());
        if (splits > 1) {
            hipLaunchKernelGGL(k_knn_merge, dim3((unsigned)((NQ + 255) / 256)), dim3(256), 0, ctx->stream, a, splits);
            OV2_HIP_CHECK(hipGetLastError());
        }
        rc = st.download(o_out, total, o_out);  if (rc) return rc;
        rc = st.sync();  if (rc) return rc;
    }
    q0 = 0;
    for (int b = 0; b < n_items; b++) {
        const size_t nq = (size_t)items[b].n_query;
        ov2_knn_result &r = results[b];
        r.n_pairs = 0;
        if (nq) {
            memcpy(r.idx, hs + o_out + 8 * q0, 8 * nq);
            memcpy(r.dist, hs + o_d + 8 * q0, 8 * nq);
            memcpy(r.good, hs + o_g + q0, nq);
            for (size_t q = 0; q < nq; q++)
                if (r.good[q]) {
                    r.pair_query[r.n_pairs] = (int)q;
                    r.pair_train[r.n_pairs] = r.idx[2 * q];
                    r.n_pairs++;
                }
        }
        q0 += nq;
    }
    return OV2_OK;
}

int ov2_knn_match(ov2_ctx *ctx, const ov2_knn_params *params, const ov2_knn_item *item, ov2_knn_result *result)
{
    OV2_REQUIRE(item && result, OV2_EINVAL, "NULL item / result");
    return ov2_knn_match_batch(ctx, params, 1, item, result);
}
