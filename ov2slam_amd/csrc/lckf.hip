// lckf.hip -- the loop closer's keyframe preparation for gfx950 (the reference's LoopCloser::run, src/loop_closer.cpp:86-144: the
// exclusion mask, FastFeatureDetector(20) on the whole raw image, KeyPointsFilter::retainBest(300), BriefDescriptorExtractor::compute).
// Semantics: include/ov2slam_hip.h ("Loop-closure keyframe preparation"); tests/lckf_ref.py is the same arithmetic in numpy.
//   k_lckf_paint   one lane per exclusion point: the filled midpoint circle as bits of a per-item mask (1 = excluded), OR-atomics
//                  on words -- an OR is the same whatever order the lanes arrive in.
//   k_lckf_fast    one work-group per LCKF_TILE_W x LCKF_TILE_H tile of one item (grid.z = item).  The tile and a 4-pixel halo (3 for
//                  the ring, 1 more because the suppression needs the neighbours' scores) go to LDS with 4-byte loads; scores are
//                  computed on the tile plus a 1-pixel halo, only where the ring test passes; then the strict 3x3 suppression and the
//                  mask bit.  Output: the item's u8 score map (survivor: its score, everything else 0), written as whole words, and
//                  the item's 256-bin histogram of surviving scores (integer atomic counts).
//   k_lckf_cut     one wavefront per item: the cut from the histogram (a suffix scan over the lanes, four bins each).
//   k_lckf_rows    one wavefront per image row: the row's counts (corners, retained, retained inside the BRIEF border).
//   k_lckf_scan    one work-group per item: exclusive prefix sums of the row counts, the item's totals.
//   k_lckf_emit    one wavefront per row: ballots give every corner its place behind the row's offset, so both lists come out in
//                  raster order and no output position depends on scheduling.
//   k_brief32      (brief.hip) on the retained points, same stream.
// Atomics touch counts only (mask bits, histogram bins); list positions come from the prefix sums.
#include "common.hpp"
#include "lckf_fast.hpp"
#include <cmath>

constexpr int LCKF_TILE_W = 64;
constexpr int LCKF_TILE_H = 16;
constexpr int LCKF_HALO = 4;                                   // 3 (ring) + 1 (the neighbours' scores)
constexpr int LCKF_PW = LCKF_TILE_W + 2 * LCKF_HALO;           // pixel tile in LDS: 72 x 24 bytes
constexpr int LCKF_PH = LCKF_TILE_H + 2 * LCKF_HALO;
constexpr int LCKF_SP = LCKF_TILE_W + 4;                       // score tile pitch: 66 columns used, padded to whole words
constexpr int LCKF_SH = LCKF_TILE_H + 2;
constexpr int LCKF_MAX_RADIUS = 64;                            // LckfArgs::hw
constexpr int LCKF_BRIEF_BORDER = 28;
static_assert(LCKF_TILE_W == 64 && LCKF_TILE_W * LCKF_TILE_H == 4 * 256, "k_lckf_fast: 256 lanes, four pixels each, one word per lane out");

struct LckfArgs {
    const uint8_t *img; long long pitch, item_stride;          // the chunk's first image
    int w, h, wide;                                            // wide: base, pitch and item stride are multiples of 4
    int threshold, retain, radius;
    const float *excl; const int *n_excl; int excl_cap;        // the chunk's first item
    // scratch, indexed by the item within the chunk
    unsigned *mask; int mwpr;                                  // bit x of row y: word y * mwpr + (x >> 5); 1 = excluded
    uint8_t *map; int mpitch;                                  // multiple of LCKF_TILE_W
    int *hist;                                                 // 256 per item
    int4 *rows;                                                // h per item: (corners, retained, retained inside the border, -)
    int *thresh;                                               // per item: the smallest retained score (256: nothing is)
    int *n_brief;                                              // per item: min(n_kept, kept_cap)
    float *fxy;                                                // kept_cap float pairs per item: k_brief32's points
    // outputs, the chunk's first item
    int16_t *all_xy; uint8_t *all_resp; int all_cap;
    int16_t *kept_xy; uint8_t *kept_resp; int kept_cap;
    int *counts;                                               // 4 per item
    signed char hw[LCKF_MAX_RADIUS + 1];                       // midpoint circle half-widths of rows +-k, -1: row not touched
};

__global__ __launch_bounds__(256) void k_lckf_paint(LckfArgs a)
{
    const int item = blockIdx.y, i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    int n = a.n_excl[item];
    n = n < a.excl_cap ? n : a.excl_cap;
    if (i >= n) return;
    const float *p = a.excl + 2 * ((long long)item * a.excl_cap + i);
    const float x = p[0], y = p[1];
    // NaN and +-inf paint nothing; nor can a centre this far out touch an image narrower than 2^15 (and the integers below stay small)
    if (!(fabsf(x) < 1048576.f) || !(fabsf(y) < 1048576.f)) return;
    const int cx = __float2int_rn(x), cy = __float2int_rn(y);           // half to even
    unsigned *mask = a.mask + (long long)item * a.h * a.mwpr;
    for (int k = -a.radius; k <= a.radius; k++) {
        const int yy = cy + k;
        if (yy < 0 || yy >= a.h) continue;
        const int half = a.hw[k < 0 ? -k : k];
        if (half < 0) continue;
        int xa = cx - half, xb = cx + half;
        if (xa >= a.w || xb < 0) continue;
        xa = xa < 0 ? 0 : xa; xb = xb > a.w - 1 ? a.w - 1 : xb;
        unsigned *row = mask + (long long)yy * a.mwpr;
        const int wa = xa >> 5, wb = xb >> 5;
        for (int wd = wa; wd <= wb; wd++) {
            const int lo = wd == wa ? (xa & 31) : 0, hi = wd == wb ? (xb & 31) : 31;
            const unsigned bits = (hi == 31 ? 0xFFFFFFFFu : ((1u << (hi + 1)) - 1u)) & ~((1u << lo) - 1u);
            atomicOr(&row[wd], bits);
        }
    }
}

__global__ __launch_bounds__(256) void k_lckf_fast(LckfArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t pix[LCKF_PH * LCKF_PW];
    __shared__ __attribute__((aligned(16))) uint8_t sc[LCKF_SH * LCKF_SP];
    __shared__ __attribute__((aligned(16))) uint8_t outb[LCKF_TILE_H * LCKF_TILE_W];
    const int tid = threadIdx.x, item = blockIdx.z;
    const int x0 = (int)blockIdx.x * LCKF_TILE_W, y0 = (int)blockIdx.y * LCKF_TILE_H;
    const uint8_t *img = a.img + (long long)item * a.item_stride;
    // the tile and its halo, a word per lane; pixels outside the image read 0 (no candidate's ring reaches them)
    for (int v = tid; v < LCKF_PH * (LCKF_PW / 4); v += 256) {
        const int r = v / (LCKF_PW / 4), c4 = v - r * (LCKF_PW / 4);
        const int gy = y0 - LCKF_HALO + r, gx = x0 - LCKF_HALO + 4 * c4;
        uint32_t word = 0;
        if (gy >= 0 && gy < a.h && gx >= 0 && gx < a.w) {
            const uint8_t *src = img + (long long)gy * a.pitch + gx;
            if (a.wide && gx + 3 < a.w) word = *(const uint32_t *)src;
            else {
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (gx + j < a.w) word |= (uint32_t)src[j] << (8 * j);
            }
        }
        ((uint32_t *)pix)[v] = word;
    }
    for (int v = tid; v < LCKF_SH * LCKF_SP / 4; v += 256) ((uint32_t *)sc)[v] = 0;
    __syncthreads();
    // scores on the tile plus one pixel around it
    for (int p = tid; p < LCKF_SH * (LCKF_TILE_W + 2); p += 256) {
        const int ry = p / (LCKF_TILE_W + 2), rx = p - ry * (LCKF_TILE_W + 2);
        const int gy = y0 - 1 + ry, gx = x0 - 1 + rx;
        if (gx < 3 || gx >= a.w - 3 || gy < 3 || gy >= a.h - 3) continue;
        const int s = lckf_fast_score<LCKF_PW>(pix + (ry + LCKF_HALO - 1) * LCKF_PW + rx + LCKF_HALO - 1, a.threshold);
        if (s) sc[ry * LCKF_SP + rx] = (uint8_t)s;
    }
    __syncthreads();
    const unsigned *mask = a.mask + (long long)item * a.h * a.mwpr;
    int *hist = a.hist + 256 * item;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int p = tid + 256 * k, ly = p / LCKF_TILE_W, lx = p - ly * LCKF_TILE_W;
        const uint8_t *c = sc + (ly + 1) * LCKF_SP + lx + 1;
        const int s = c[0];
        bool keep = s > 0 && s > c[-1] && s > c[1] && s > c[-LCKF_SP - 1] && s > c[-LCKF_SP] && s > c[-LCKF_SP + 1] &&
                    s > c[LCKF_SP - 1] && s > c[LCKF_SP] && s > c[LCKF_SP + 1];
        if (keep) {                                                    // (a score was only written inside the image)
            const int gx = x0 + lx, gy = y0 + ly;
            keep = ((mask[(long long)gy * a.mwpr + (gx >> 5)] >> (gx & 31)) & 1u) == 0;
        }
        if (keep) atomicAdd(&hist[s], 1);
        outb[p] = keep ? (uint8_t)s : 0;
    }
    __syncthreads();
    const int row = tid >> 4, gy = y0 + row;                           // 16 words per tile row
    if (gy < a.h)
        ((uint32_t *)(a.map + ((long long)item * a.h + gy) * a.mpitch + x0))[tid & 15] = ((const uint32_t *)outb)[tid];
}

// KeyPointsFilter::retainBest on the histogram of byte responses, one wavefront per item: lane l holds bins 4l .. 4l+3, a suffix
// scan over the lanes gives every bin the number of responses at or above it.  thresh: the smallest retained score (256: none);
// cut: what the caller is told (0 when nothing was cut).
__global__ __launch_bounds__(256) void k_lckf_cut(LckfArgs a, int n_items)
{
    const int lane = threadIdx.x & 63, item = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (item >= n_items) return;
    const int4 hb = ((const int4 *)(a.hist + 256 * item))[lane];      // (bin 0 is never counted: a survivor scores at least 1)
    const int mine = hb.x + hb.y + hb.z + hb.w;
    int suf = mine;                                                    // bins of this lane and of every higher lane
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_down(suf, o);
        if (lane + o < 64) suf += v;
    }
    const int tot = __shfl(suf, 0);
    const int c3 = suf - mine + hb.w, c2 = c3 + hb.z, c1 = c2 + hb.y, c0 = c1 + hb.x;      // responses >= 4l+3, 4l+2, 4l+1, 4l
    const int r = a.retain;
    int best = c3 >= r ? 4 * lane + 3 : (c2 >= r ? 4 * lane + 2 : (c1 >= r ? 4 * lane + 1 : (c0 >= r ? 4 * lane : -1)));
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) best = max(best, __shfl_xor(best, o));
    if (lane == 0) {
        int cut = 0, thresh = 1;
        if (r == 0) thresh = 256;
        else if (r > 0 && tot > r) { cut = best; thresh = best; }
        a.thresh[item] = thresh;
        a.counts[4 * item + 1] = cut;
    }
}

__device__ __forceinline__ int lckf_wave_sum(int v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(256) void k_lckf_rows(LckfArgs a)
{
    const int item = blockIdx.y, lane = threadIdx.x & 63;
    const int y = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (y >= a.h) return;
    const int thresh = a.thresh[item];
    const uint8_t *row = a.map + ((long long)item * a.h + y) * a.mpitch;
    const bool yin = y >= LCKF_BRIEF_BORDER && y < a.h - LCKF_BRIEF_BORDER;
    int n_all = 0, n_kept = 0, n_desc = 0;
    for (int x0 = 0; x0 < a.mpitch; x0 += 256) {
        const int x = x0 + 4 * lane;
        const uint32_t word = x < a.mpitch ? *(const uint32_t *)(row + x) : 0u;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int s = (word >> (8 * j)) & 0xff;
            n_all += s != 0;
            n_kept += s >= thresh;
            n_desc += s >= thresh && yin && x + j >= LCKF_BRIEF_BORDER && x + j < a.w - LCKF_BRIEF_BORDER;
        }
    }
    n_all = lckf_wave_sum(n_all); n_kept = lckf_wave_sum(n_kept); n_desc = lckf_wave_sum(n_desc);
    if (lane == 0) a.rows[(long long)item * a.h + y] = make_int4(n_all, n_kept, n_desc, 0);
}

__global__ __launch_bounds__(256) void k_lckf_scan(LckfArgs a)
{
    __shared__ int s[3][256];
    const int item = blockIdx.x, tid = threadIdx.x;
    int4 *rows = a.rows + (long long)item * a.h;
    int base[3] = {0, 0, 0};
    for (int r0 = 0; r0 < a.h; r0 += 256) {
        const int y = r0 + tid;
        const int4 v = y < a.h ? rows[y] : make_int4(0, 0, 0, 0);
        s[0][tid] = v.x; s[1][tid] = v.y; s[2][tid] = v.z;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            int t[3] = {0, 0, 0};
            if (tid >= o) { t[0] = s[0][tid - o]; t[1] = s[1][tid - o]; t[2] = s[2][tid - o]; }
            __syncthreads();
            s[0][tid] += t[0]; s[1][tid] += t[1]; s[2][tid] += t[2];
            __syncthreads();
        }
        if (y < a.h) rows[y] = make_int4(base[0] + s[0][tid] - v.x, base[1] + s[1][tid] - v.y, base[2] + s[2][tid] - v.z, 0);
        const int t0 = s[0][255], t1 = s[1][255], t2 = s[2][255];
        __syncthreads();
        base[0] += t0; base[1] += t1; base[2] += t2;
    }
    if (tid == 0) {
        int *c = a.counts + 4 * item;                                  // (c[1], the cut, is k_lckf_cut's)
        c[0] = base[0]; c[2] = base[1]; c[3] = base[2];
        a.n_brief[item] = base[1] < a.kept_cap ? base[1] : a.kept_cap;
    }
}

__global__ __launch_bounds__(256) void k_lckf_emit(LckfArgs a)
{
    const int item = blockIdx.y, lane = threadIdx.x & 63;
    const int y = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (y >= a.h) return;
    const int thresh = a.thresh[item];
    const int4 off = a.rows[(long long)item * a.h + y];
    const uint8_t *row = a.map + ((long long)item * a.h + y) * a.mpitch;
    const unsigned long long below = (1ull << lane) - 1ull;
    int run_all = off.x, run_kept = off.y;
    for (int x0 = 0; x0 < a.mpitch; x0 += 256) {
        const int x = x0 + 4 * lane;
        const uint32_t word = x < a.mpitch ? *(const uint32_t *)(row + x) : 0u;
        unsigned long long ba[4], bk[4];
        int pre_all = 0, pre_kept = 0, tot_all = 0, tot_kept = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int s = (word >> (8 * j)) & 0xff;
            ba[j] = __ballot(s != 0); bk[j] = __ballot(s >= thresh);
            pre_all += __popcll(ba[j] & below); pre_kept += __popcll(bk[j] & below);
            tot_all += __popcll(ba[j]); tot_kept += __popcll(bk[j]);
        }
        if (tot_all == 0) continue;                                    // (wave-uniform)
#pragma unroll
        for (int j = 0; j < 4; j++) {                                  // the lane's own four pixels, left to right
            const int s = (word >> (8 * j)) & 0xff;
            if (s != 0) {
                const long long pa = (long long)run_all + pre_all;
                if (pa < a.all_cap) {
                    const long long o = (long long)item * a.all_cap + pa;
                    a.all_xy[2 * o] = (int16_t)(x + j); a.all_xy[2 * o + 1] = (int16_t)y; a.all_resp[o] = (uint8_t)s;
                }
                pre_all++;
            }
            if (s >= thresh) {
                const long long pk = (long long)run_kept + pre_kept;
                if (pk < a.kept_cap) {
                    const long long o = (long long)item * a.kept_cap + pk;
                    a.kept_xy[2 * o] = (int16_t)(x + j); a.kept_xy[2 * o + 1] = (int16_t)y; a.kept_resp[o] = (uint8_t)s;
                    a.fxy[2 * o] = (float)(x + j); a.fxy[2 * o + 1] = (float)y;
                }
                pre_kept++;
            }
        }
        run_all += tot_all; run_kept += tot_kept;
    }
}


// drawing.cpp Circle(): rows +-dy get half-width dx, rows +-dx get dy (the fill variant's four spans per step)
static void lckf_halfwidths(signed char *hw, int radius)
{
    for (int k = 0; k <= LCKF_MAX_RADIUS; k++) hw[k] = -1;
    int err = 0, dx = radius, dy = 0, plus = 1, minus = (radius << 1) - 1;
    while (dx >= dy) {
        if (dx > hw[dy]) hw[dy] = (signed char)dx;
        if (dy > hw[dx]) hw[dx] = (signed char)dy;
        dy++;
        err += plus;
        plus += 2;
        const int m = (err <= 0) - 1;
        err -= minus & m;
        dx += m;
        minus -= m & 2;
    }
}

static int lckf_check_params(const ov2_lckf_params *params)
{
    OV2_REQUIRE(params, OV2_EINVAL, "NULL params");
    OV2_REQUIRE(params->excl_radius >= 0 && params->excl_radius <= LCKF_MAX_RADIUS, OV2_EINVAL, "excl_radius outside [0, 64]");
    return OV2_OK;
}
static int lckf_check_geometry(int w, int h, long long pitch, size_t item_stride, int n_items)
{
    OV2_REQUIRE(w >= 1 && h >= 1, OV2_EINVAL, "image size below 1");
    OV2_REQUIRE(w < 32768 && h < 32768, OV2_EUNSUPPORTED, "an image side of 2^15 or more (int16 coordinates)");
    OV2_REQUIRE(pitch >= (long long)w, OV2_EINVAL, "stride < width");
    OV2_REQUIRE(n_items >= 0, OV2_EINVAL, "n_items < 0");
    OV2_REQUIRE(n_items <= 65535, OV2_EUNSUPPORTED, "more than 65535 items in one call");
    OV2_REQUIRE(n_items <= 1 || item_stride >= (size_t)pitch * (size_t)h, OV2_EINVAL, "item_stride smaller than one image");
    return OV2_OK;
}
static int lckf_check_result(const ov2_lckf_result *r)
{
    OV2_REQUIRE(r->all_cap >= 0 && r->kept_cap >= 0, OV2_EINVAL, "negative capacity (all_cap / kept_cap)");
    OV2_REQUIRE(r->all_cap == 0 || (r->all_xy && r->all_resp), OV2_EINVAL, "NULL result buffer (all_xy / all_resp)");
    OV2_REQUIRE(r->kept_cap == 0 || (r->kept_xy && r->kept_resp && r->kept_valid && r->kept_desc), OV2_EINVAL,
                "NULL result buffer (kept_xy / kept_resp / kept_valid / kept_desc)");
    return OV2_OK;
}

// The scratch of one chunk of items and how many items a chunk holds under the context's budget (OV2_OPT_LCKF_SCRATCH_KB)
struct LckfPlan { size_t per_item, o_mask, o_hist, o_map, o_rows, o_th, o_nb, o_fxy, total; int chunk, mpitch, mwpr; };
static LckfPlan lckf_plan(const ov2_ctx *ctx, int w, int h, int n_items, int kept_cap)
{
    LckfPlan p;
    p.mpitch = (w + LCKF_TILE_W - 1) / LCKF_TILE_W * LCKF_TILE_W;
    p.mwpr = (w + 31) / 32;
    const size_t b_mask = up256(4 * (size_t)p.mwpr * h), b_hist = 1024, b_map = up256((size_t)p.mpitch * h), b_rows = up256(16 * (size_t)h);
    const size_t b_fxy = up256(8 * (size_t)kept_cap);
    p.per_item = b_mask + b_hist + b_map + b_rows + 8 + b_fxy;
    size_t chunk = ((size_t)ctx->lckf_scratch_kb << 10) / p.per_item;
    chunk = chunk < 1 ? 1 : chunk;
    p.chunk = (int)(chunk < (size_t)n_items ? chunk : (size_t)(n_items > 0 ? n_items : 1));
    const size_t c = (size_t)p.chunk;
    // [masks][histograms]: one memset per chunk; then the maps, the row counts, the two small per-item arrays, BRIEF's points
    p.o_mask = 0; p.o_hist = b_mask * c; p.o_map = p.o_hist + b_hist * c; p.o_rows = p.o_map + b_map * c;
    p.o_th = p.o_rows + b_rows * c; p.o_nb = up256(p.o_th + 4 * c); p.o_fxy = up256(p.o_nb + 4 * c);
    p.total = p.o_fxy + b_fxy * c;
    return p;
}

// Everything on the device, enqueued on the context's stream, no synchronisation.  scratch: pl.total bytes.
static int lckf_run_d(ov2_ctx *ctx, const LckfPlan &pl, uint8_t *scratch, const ov2_lckf_params *params, const uint8_t *img_d, int w, int h,
                      size_t pitch, size_t item_stride, int n_items, const float *excl_d, int excl_cap, const int *n_excl_d,
                      int16_t *all_xy, uint8_t *all_resp, int all_cap, int16_t *kept_xy, uint8_t *kept_resp, uint8_t *kept_valid,
                      uint8_t *kept_desc, int kept_cap, int *counts)
{
    LckfArgs a;
    memset(&a, 0, sizeof(a));
    a.pitch = (long long)pitch; a.item_stride = n_items > 1 ? (long long)item_stride : 0;
    a.w = w; a.h = h;
    a.wide = ((uintptr_t)img_d % 4 == 0 && pitch % 4 == 0 && (n_items <= 1 || item_stride % 4 == 0)) ? 1 : 0;
    a.threshold = params->threshold < 0 ? 0 : (params->threshold > 255 ? 255 : params->threshold);
    a.retain = params->retain; a.radius = params->excl_radius;
    a.excl_cap = excl_cap;
    a.mwpr = pl.mwpr; a.mpitch = pl.mpitch;
    a.mask = (unsigned *)(scratch + pl.o_mask); a.hist = (int *)(scratch + pl.o_hist); a.map = scratch + pl.o_map;
    a.rows = (int4 *)(scratch + pl.o_rows); a.thresh = (int *)(scratch + pl.o_th); a.n_brief = (int *)(scratch + pl.o_nb);
    a.fxy = (float *)(scratch + pl.o_fxy);
    a.all_cap = all_cap; a.kept_cap = kept_cap;
    lckf_halfwidths(a.hw, a.radius);
    const dim3 tiles((unsigned)(pl.mpitch / LCKF_TILE_W), (unsigned)((h + LCKF_TILE_H - 1) / LCKF_TILE_H));
    const unsigned row_groups = (unsigned)((h + 3) / 4);
    for (int b0 = 0; b0 < n_items; b0 += pl.chunk) {                   // every chunk reuses the scratch: the stream orders them
        const int nb = n_items - b0 < pl.chunk ? n_items - b0 : pl.chunk;
        a.img = img_d + (size_t)b0 * (n_items > 1 ? item_stride : 0);
        a.excl = excl_d ? excl_d + 2 * (size_t)b0 * excl_cap : nullptr; a.n_excl = n_excl_d ? n_excl_d + b0 : nullptr;
        a.all_xy = all_xy ? all_xy + 2 * (size_t)b0 * all_cap : nullptr; a.all_resp = all_resp ? all_resp + (size_t)b0 * all_cap : nullptr;
        a.kept_xy = kept_xy ? kept_xy + 2 * (size_t)b0 * kept_cap : nullptr; a.kept_resp = kept_resp ? kept_resp + (size_t)b0 * kept_cap : nullptr;
        a.counts = counts + 4 * (size_t)b0;
        OV2_HIP_CHECK(hipMemsetAsync(scratch + pl.o_mask, 0, pl.o_map - pl.o_mask, ctx->stream));
        if (excl_cap > 0 && excl_d && n_excl_d) {
            hipLaunchKernelGGL(k_lckf_paint, dim3((unsigned)((excl_cap + 255) / 256), (unsigned)nb), dim3(256), 0, ctx->stream, a);
            OV2_HIP_CHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_lckf_fast, dim3(tiles.x, tiles.y, (unsigned)nb), dim3(256), 0, ctx->stream, a);
        OV2_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_lckf_cut, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, ctx->stream, a, nb);
        OV2_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_lckf_rows, dim3(row_groups, (unsigned)nb), dim3(256), 0, ctx->stream, a);
        OV2_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_lckf_scan, dim3((unsigned)nb), dim3(256), 0, ctx->stream, a);
        OV2_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_lckf_emit, dim3(row_groups, (unsigned)nb), dim3(256), 0, ctx->stream, a);
        OV2_HIP_CHECK(hipGetLastError());
        if (kept_cap > 0) {
            const int rc = ov2_brief_launch_d(ctx, a.img, w, h, pitch, n_items > 1 ? item_stride : 0, nb, a.fxy, kept_cap, a.n_brief, 0,
                                              kept_desc + 32 * (size_t)b0 * kept_cap, kept_valid + (size_t)b0 * kept_cap);
            if (rc != OV2_OK) return rc;
        }
    }
    return OV2_OK;
}

int ov2_lckf_run_h(ov2_ctx *ctx, const uint8_t *img_h, const uint8_t *img_d, int w, int h, size_t pitch, size_t item_stride, int n_items,
                   const ov2_lckf_params *params, const float *excl_xy_h, const int *n_excl_h, int excl_cap, ov2_lckf_result *results)
{
    // the inputs first, the context last: a malformed input is reported without a device
    int rc = lckf_check_params(params);
    if (rc != OV2_OK) return rc;
    rc = lckf_check_geometry(w, h, (long long)pitch, item_stride, n_items);
    if (rc != OV2_OK) return rc;
    OV2_REQUIRE(n_items >= 1, OV2_EINVAL, "n_items < 1");
    OV2_REQUIRE(results && n_excl_h, OV2_EINVAL, "NULL result / count array");
    OV2_REQUIRE(excl_cap >= 0, OV2_EINVAL, "negative count (excl_cap)");
    int all_cap = 0, kept_cap = 0;
    for (int b = 0; b < n_items; b++) {
        OV2_REQUIRE(n_excl_h[b] >= 0 && n_excl_h[b] <= excl_cap, OV2_EINVAL, "negative count (n_excl), or more points than slots");
        OV2_REQUIRE(n_excl_h[b] == 0 || excl_xy_h, OV2_EINVAL, "excl_xy == NULL");
        rc = lckf_check_result(&results[b]);
        if (rc != OV2_OK) return rc;
        all_cap = results[b].all_cap > all_cap ? results[b].all_cap : all_cap;
        kept_cap = results[b].kept_cap > kept_cap ? results[b].kept_cap : kept_cap;
    }
    OV2_REQUIRE(ctx, OV2_EINVAL, "NULL context");
    OV2_HIP_CHECK(hipSetDevice(ctx->device));
    // staging, the same layout on both sides: [n_excl 4][excl 8 per slot] | [counts 16][kept_xy 4][kept_resp 1][kept_valid 1][kept_desc 32]
    // [all_xy 4][all_resp 1] per slot; on the device the host image (if any) ahead of it and the scratch behind
    const size_t B = (size_t)n_items, ks = B * (size_t)kept_cap, as = B * (size_t)all_cap;
    const size_t o_n = 0, o_ex = up256(4 * B), o_out = up256(o_ex + 8 * B * (size_t)excl_cap);
    const size_t o_kxy = up256(o_out + 16 * B), o_kr = up256(o_kxy + 4 * ks), o_kv = up256(o_kr + ks), o_kd = up256(o_kv + ks);
    const size_t o_axy = up256(o_kd + 32 * ks), o_ar = up256(o_axy + 4 * as), blk = up256(o_ar + as);
    const size_t img_pitch = up256((size_t)w), img_bytes = img_h ? up256(img_pitch * (size_t)h) : 0;
    const LckfPlan pl = lckf_plan(ctx, w, h, n_items, kept_cap);
    rc = ctx->reserve_host(blk);                                                  if (rc != OV2_OK) return rc;
    rc = ctx->reserve_device(img_bytes + blk + pl.total);           if (rc != OV2_OK) return rc;
    uint8_t *dimg = (uint8_t *)ctx->d_scratch, *dblk = dimg + img_bytes, *hblk = (uint8_t *)ctx->h_scratch;
    if (img_h) {
        rc = ctx->upload_image(dimg, img_pitch, img_h, pitch, (size_t)w, (size_t)h);
        if (rc != OV2_OK) return rc;
        img_d = dimg; pitch = img_pitch; item_stride = img_bytes;
    }
    for (int b = 0; b < n_items; b++) {
        ((int *)(hblk + o_n))[b] = n_excl_h[b];
        if (n_excl_h[b]) memcpy(hblk + o_ex + 8 * (size_t)b * excl_cap, excl_xy_h + 2 * (size_t)b * excl_cap, 8 * (size_t)n_excl_h[b]);
    }
    OV2_HIP_CHECK(hipMemcpyAsync(dblk, hblk, o_out, hipMemcpyHostToDevice, ctx->stream));
    rc = lckf_run_d(ctx, pl, dblk + blk, params, img_d, w, h, pitch, item_stride, n_items, (const float *)(dblk + o_ex), excl_cap,
                    (const int *)(dblk + o_n), (int16_t *)(dblk + o_axy), dblk + o_ar, all_cap, (int16_t *)(dblk + o_kxy), dblk + o_kr,
                    dblk + o_kv, dblk + o_kd, kept_cap, (int *)(dblk + o_out));
    if (rc != OV2_OK) return rc;
    OV2_HIP_CHECK(hipMemcpyAsync(hblk + o_out, dblk + o_out, blk - o_out, hipMemcpyDeviceToHost, ctx->stream));
    OV2_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (int b = 0; b < n_items; b++) {
        ov2_lckf_result &r = results[b];
        const int *c = (const int *)(hblk + o_out) + 4 * b;
        r.n_all = c[0]; r.cut = c[1]; r.n_kept = c[2]; r.n_desc = c[3];
        const size_t na = (size_t)(r.n_all < r.all_cap ? r.n_all : r.all_cap), nk = (size_t)(r.n_kept < r.kept_cap ? r.n_kept : r.kept_cap);
        const size_t oa = (size_t)b * all_cap, ok = (size_t)b * kept_cap;
        if (na) { memcpy(r.all_xy, hblk + o_axy + 4 * oa, 4 * na); memcpy(r.all_resp, hblk + o_ar + oa, na); }
        if (nk) {
            memcpy(r.kept_xy, hblk + o_kxy + 4 * ok, 4 * nk); memcpy(r.kept_resp, hblk + o_kr + ok, nk);
            memcpy(r.kept_valid, hblk + o_kv + ok, nk); memcpy(r.kept_desc, hblk + o_kd + 32 * ok, 32 * nk);
        }
    }
    return OV2_OK;
}

extern "C" {

int ov2_lckf_params_init(ov2_lckf_params *out)
{
    OV2_REQUIRE(out, OV2_EINVAL, "NULL params");
    out->threshold = 20; out->retain = 300; out->excl_radius = 2;          // src/loop_closer.cpp:119, :123, :110
    return OV2_OK;
}

int ov2_lckf_prepare(ov2_ctx *ctx, const uint8_t *img_h, int w, int h, int stride, const ov2_lckf_params *params,
                     const float *excl_xy_h, int n_excl, ov2_lckf_result *result)
{
    OV2_REQUIRE(img_h && result, OV2_EINVAL, "NULL image / result");
    OV2_REQUIRE(n_excl >= 0, OV2_EINVAL, "negative count (n_excl)");
    return ov2_lckf_run_h(ctx, img_h, nullptr, w, h, (size_t)(stride > 0 ? stride : 0), 0, 1, params, excl_xy_h, &n_excl, n_excl, result);
}

int ov2_lckf_prepare_batch_d(ov2_ctx *ctx, const ov2_lckf_params *params, const uint8_t *img_d, int w, int h, int pitch,
                             size_t item_stride, int n_items, const float *excl_xy_d, int excl_cap, const int *n_excl_d,
                             int16_t *all_xy_d, uint8_t *all_resp_d, int all_cap, int16_t *kept_xy_d, uint8_t *kept_resp_d,
                             uint8_t *kept_valid_d, uint8_t *kept_desc_d, int kept_cap, int *counts_d)
{
    int rc = lckf_check_params(params);
    if (rc != OV2_OK) return rc;
    rc = lckf_check_geometry(w, h, (long long)pitch, item_stride, n_items);
    if (rc != OV2_OK) return rc;
    OV2_REQUIRE(excl_cap >= 0 && all_cap >= 0 && kept_cap >= 0, OV2_EINVAL, "negative capacity (excl_cap / all_cap / kept_cap)");
    if (n_items > 0) {
        OV2_REQUIRE(img_d && counts_d, OV2_EINVAL, "NULL device buffer (img / counts)");
        OV2_REQUIRE(excl_cap == 0 || (excl_xy_d && n_excl_d), OV2_EINVAL, "NULL device buffer (excl_xy / n_excl)");
        OV2_REQUIRE(all_cap == 0 || (all_xy_d && all_resp_d), OV2_EINVAL, "NULL device buffer (all_xy / all_resp)");
        OV2_REQUIRE(kept_cap == 0 || (kept_xy_d && kept_resp_d && kept_valid_d && kept_desc_d), OV2_EINVAL,
                    "NULL device buffer (kept_xy / kept_resp / kept_valid / kept_desc)");
    }
    OV2_REQUIRE(ctx, OV2_EINVAL, "NULL context");
    if (n_items == 0) return OV2_OK;
    OV2_HIP_CHECK(hipSetDevice(ctx->device));
    const LckfPlan pl = lckf_plan(ctx, w, h, n_items, kept_cap);
    rc = ctx->reserve_device(pl.total);
    if (rc != OV2_OK) return rc;
    rc = lckf_run_d(ctx, pl, (uint8_t *)ctx->d_scratch, params, img_d, w, h, (size_t)pitch, item_stride, n_items, excl_xy_d, excl_cap, n_excl_d,
                    all_xy_d, all_resp_d, all_cap, kept_xy_d, kept_resp_d, kept_valid_d, kept_desc_d, kept_cap, counts_d);
    if (rc != OV2_OK) return rc;
    OV2_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return OV2_OK;
}

} // extern "C"
