// gftt.hip -- FeatureExtractor::detectGFTT (the reference's src/feature_extractor.cpp:104-221) and setMask (:575-584) for gfx950:
// cv::goodFeaturesToTrack (minimum-eigenvalue response, no Harris, blockSize 3, gradientSize 3) run once or twice per image, as
// restated from the public OpenCV 4.x source (imgproc/src/featureselect.cpp, corner.cpp, box_filter.cpp); see include/ov2slam_hip.h.
//
// Per pass and image (one chunk of batch items at a time, every launch covering the whole chunk):
//   k_gftt_mask_init / k_gftt_circles   the mask: roi (or all ones), zeroed by filled cv::circle discs (d_circle_halfwidths)
//   k_gftt_eig                          [once] cornerMinEigenVal on the whole image: one thread per column sweeps it top to bottom,
//                                       so the double sliding column sum rounds along the same path as OpenCV's ColumnSum
//   k_gftt_max                          minMaxLoc(eig, mask): atomicMax of an order-preserving integer image of the float
//   k_gftt_rows / k_gftt_scan / k_gftt_write   threshold + 3x3 dilate + mask -> candidates, compacted per row in DESCENDING
//                                       offset order (one wavefront per row, then an exclusive scan over the rows)
//   k_gftt_sort                         one work-group per item: stable LSD radix sort (8-bit digits) on the value alone; stability
//                                       keeps equal values in descending offset order = OpenCV 4.x greaterThanPtr
//   k_gftt_walk                         one wavefront per item: the greedy minimum-distance pass, 64 candidates per step tested
//                                       against the accepted points (a cell grid of linked lists in LDS), conflicts inside a step
//                                       resolved in lane order (ballot + readlane)
//   launch_subpix                       cv::cornerSubPix on the accepted points (device-side counts)
// Pass 2 runs for every item; its kernels leave at once where the walk of pass 1 did not set the item's flag.  k_gftt_append
// concatenates the two lists.  One host synchronisation per call.
#include "common.hpp"
#include <math.h>
#include <algorithm>

#pragma clang fp contract(off)

#define GFTT_MAX_CORNERS 4096          // points one pass may accept (the walk's LDS list); nb2detect above -> OV2_EUNSUPPORTED
#define GFTT_GRID_MAX 8192             // cells of the walk's LDS grid (the cell side grows past minDistance until it fits)
#define GFTT_MAX_RADIUS 63             // d_circle_halfwidths' table
#define GFTT_SCRATCH_BUDGET (256ull << 20)    // bytes of per-item scratch a chunk may use (at least one item)

// per item, per call (device)
struct GfttItem {
    unsigned maxbits[2];   // per pass: order-preserving image of the masked maximum (0: no pixel under the mask -> maxVal 0)
    int nb2d;              // nb2detect (0: nothing to detect -- early return or no work)
    int n1, n2;            // points accepted by pass 1 / pass 2
    int pass2;             // pass 2 runs
    int ncand;             // candidates of the current pass
    int sorted_b;          // the sorted candidates of the current pass are in buffer B
};

struct GfttArgs {
    int w, h, stride;              // image geometry (rows `stride` bytes apart)
    long long img_item_stride;     // bytes between the items' images
    const uint8_t *img;            // item 0
    const uint8_t *roi; int roi_stride;   // shared by every item; NULL: all pixels
    const float2 *cur; int cur_cap; const int *ncur; int ncur_all;   // current keypoints (ncur NULL: ncur_all each)
    const int *nbmax;              // per item
    int nmaxpts, nmaxdist, nmindist;
    double q1, q2;                 // dminquality, dmaxquality
    int sobel_dy_order;
    // chunk scratch (per item strides)
    float *eig; long long px_stride;                         // w*h floats per item (rounded)
    uint8_t *mask; long long mask_stride;                    // w*h bytes per item (rounded)
    unsigned *keyA, *valA, *keyB, *valB; long long cand_stride;   // (w-2)*(h-2)
    int *rowcnt; int row_stride;                             // h
    float2 *out; int out_cap;                                // final list (pass 1 is written here directly)
    float2 *out2;                                            // pass-2 list, out_cap slots per item
    GfttItem *it;
};

__device__ __forceinline__ int g_reflect101(int p, int len)
{
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - 2 - p;
    return p;
}

// order-preserving map float -> unsigned (for non-NaN values)
__device__ __forceinline__ unsigned g_ord(float f)
{
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float g_unord(unsigned o)
{
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// midpoint circle half-widths (drawing.cpp Circle()), as in detect.hip: hw[k] for rows +-k, -1 = row not touched
__device__ __forceinline__ void g_circle_halfwidths(int *hw, int radius)
{
    for (int k = 0; k < 64; k++) hw[k] = -1;
    int err = 0, dx = radius, dy = 0, plus = 1, minus = (radius << 1) - 1;
    while (dx >= dy) {
        if (dx > hw[dy]) hw[dy] = dx;
        if (dy > hw[dx]) hw[dx] = dy;
        dy++; err += plus; plus += 2;
        const int m = (err <= 0) - 1;
        err -= minus & m; dx += m; minus -= m & 2;
    }
}

// current keypoints of an item (a device count is clamped to the list's capacity)
__device__ __forceinline__ int g_ncur(const GfttArgs &A, int item)
{
    const int n = A.ncur ? A.ncur[item] : A.ncur_all;
    return A.cur ? min(max(n, 0), A.cur_cap) : 0;
}

__device__ __forceinline__ bool g_active(const GfttArgs &A, int item, int pass)
{
    const GfttItem &I = A.it[item];
    return I.nb2d > 0 && (pass == 0 || I.pass2);
}

// (float)(maxVal * quality): threshold(eig, eig, maxVal*quality, 0, THRESH_TOZERO) on a CV_32F image
__device__ __forceinline__ float g_thresh(const GfttArgs &A, int item, int pass)
{
    const unsigned mb = A.it[item].maxbits[pass];
    const double mx = mb ? (double)g_unord(mb) : 0.0;
    return (float)(mx * (pass == 0 ? A.q1 : A.q2));
}

// candidate: val != 0 && val == dilate(val) && mask, val the thresholded response (interior pixels only)
__device__ __forceinline__ bool g_is_cand(const float *E, const uint8_t *M, int w, int x, int y, float thr, float *val)
{
    const float *r = E + (long long)y * w + x;
    const float c0 = r[0];
    const float c = c0 > thr ? c0 : 0.f;
    *val = c;
    if (c == 0.f || M[(long long)y * w + x] == 0) return false;
    bool ok = true;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const float v = r[dy * w + dx];
            const float t = v > thr ? v : 0.f;
            ok = ok && !(t > c);
        }
    return ok;
}

// nb2detect per item (:108-116); the header is cleared
__global__ void k_gftt_setup(GfttArgs A, int items)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= items) return;
    const int ncur = g_ncur(A, i);
    const int nbmax = A.nbmax[i];
    GfttItem I;
    I.maxbits[0] = I.maxbits[1] = 0u;
    I.nb2d = ncur >= A.nmaxpts ? 0 : (nbmax != -1 ? nbmax : A.nmaxpts - ncur);
    I.n1 = I.n2 = I.pass2 = I.ncand = I.sorted_b = 0;
    A.it[i] = I;
}

__global__ __launch_bounds__(256) void k_gftt_mask_init(GfttArgs A, int pass)
{
    const int item = blockIdx.y;
    if (!g_active(A, item, pass)) return;
    const long long npx = (long long)A.w * A.h;
    uint8_t *M = A.mask + item * A.mask_stride;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < npx; p += (long long)gridDim.x * 256) {
        const int y = (int)(p / A.w), x = (int)(p - (long long)y * A.w);
        M[p] = A.roi ? (A.roi[(long long)y * A.roi_stride + x] != 0) : 1;
    }
}

// one wavefront per disc: the current keypoints (both passes), then the pass-1 points (pass 2); centre cvRound(x), cvRound(y)
__global__ __launch_bounds__(64) void k_gftt_circles(GfttArgs A, int pass)
{
    const int item = blockIdx.y, p = blockIdx.x, lane = threadIdx.x;
    if (!g_active(A, item, pass)) return;
    const int ncur = g_ncur(A, item);
    float2 c;
    if (p < ncur) c = A.cur[(long long)item * A.cur_cap + p];
    else if (pass == 1 && p - ncur < A.it[item].n1) c = A.out[(long long)item * A.out_cap + (p - ncur)];
    else return;
    if (!(fabsf(c.x) < 1e7f && fabsf(c.y) < 1e7f)) return;          // (NaN, inf and far-away centres draw nothing inside the image)
    const int cx = (int)rintf(c.x), cy = (int)rintf(c.y);
    const int radius = pass == 0 ? A.nmaxdist : A.nmindist;
    __shared__ int hw[64];
    if (lane == 0) g_circle_halfwidths(hw, radius);
    __syncthreads();
    uint8_t *M = A.mask + item * A.mask_stride;
    for (int r = -radius; r <= radius; r++) {
        const int y = cy + r, k = r < 0 ? -r : r;
        if (y < 0 || y >= A.h || hw[k] < 0) continue;
        const int x0 = max(cx - hw[k], 0), x1 = min(cx + hw[k], A.w - 1);
        for (int x = x0 + lane; x <= x1; x += 64) M[(long long)y * A.w + x] = 0;
    }
}

// cornerMinEigenVal(im, eig, 3, 3), REFLECT_101 at the image border.  One thread per column, rows top to bottom.
__global__ __launch_bounds__(64) void k_gftt_eig(GfttArgs A)
{
    const int item = blockIdx.y, x = blockIdx.x * 64 + threadIdx.x;
    if (A.it[item].nb2d <= 0 || x >= A.w) return;
    const int w = A.w, h = A.h;
    const uint8_t *img = A.img + item * A.img_item_stride;
    float *E = A.eig + item * A.px_stride;
    const float f1 = (float)(1.0 / (4.0 * 3.0 * 255.0)), f0 = (float)(2.0 * (1.0 / (4.0 * 3.0 * 255.0)));
    // the three derivative columns of the row sum (reflected), and the three pixel columns of each
    int dc[3], pc[3][3];
    dc[0] = g_reflect101(x - 1, w); dc[1] = x; dc[2] = g_reflect101(x + 1, w);
#pragma unroll
    for (int k = 0; k < 3; k++) { pc[k][0] = g_reflect101(dc[k] - 1, w); pc[k][1] = dc[k]; pc[k][2] = g_reflect101(dc[k] + 1, w); }
    const bool exact = A.sobel_dy_order == OV2_SOBEL_DY_EXACT_SUM;
    // RowSum<float, double> of (dx*dx, dx*dy, dy*dy) at derivative row yy (already reflected)
    auto rowsum = [&](int yy, double (&s)[3]) {
        const uint8_t *rm = img + (long long)g_reflect101(yy - 1, h) * A.stride;
        const uint8_t *r0 = img + (long long)yy * A.stride;
        const uint8_t *rp = img + (long long)g_reflect101(yy + 1, h) * A.stride;
        int P[3][3][3];                 // [column k][row][pixel column]
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
            for (int j = 0; j < 3; j++) { P[k][0][j] = rm[pc[k][j]]; P[k][1][j] = r0[pc[k][j]]; P[k][2][j] = rp[pc[k][j]]; }
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float a0 = (float)(P[k][0][2] - P[k][0][0]), a1 = (float)(P[k][1][2] - P[k][1][0]), a2 = (float)(P[k][2][2] - P[k][2][0]);
            const float dx = (a0 + a2) * f1 + a1 * f0;
            float dy;
            if (exact) {
                const float s0 = (float)(P[k][0][0] + 2 * P[k][0][1] + P[k][0][2]);
                const float s2 = (float)(P[k][2][0] + 2 * P[k][2][1] + P[k][2][2]);
                dy = (s2 - s0) * f1;
            } else {
                const float s0 = ((float)P[k][0][0] * f1 + (float)P[k][0][1] * f0) + (float)P[k][0][2] * f1;
                const float s2 = ((float)P[k][2][0] * f1 + (float)P[k][2][1] * f0) + (float)P[k][2][2] * f1;
                dy = s2 - s0;
            }
            const float v0 = dx * dx, v1 = dx * dy, v2 = dy * dy;
            if (k == 0) { s[0] = (double)v0; s[1] = (double)v1; s[2] = (double)v2; }
            else { s[0] += (double)v0; s[1] += (double)v1; s[2] += (double)v2; }
        }
    };
    double rm1[3], r0[3], rp1[3], SUM[3];
    rowsum(g_reflect101(-1, h), rm1);
    rowsum(0, r0);
#pragma unroll
    for (int c = 0; c < 3; c++) { SUM[c] = 0.0; SUM[c] += rm1[c]; SUM[c] += r0[c]; }
    for (int y = 0; y < h; y++) {
        rowsum(g_reflect101(y + 1, h), rp1);
        float cov[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double s0 = SUM[c] + rp1[c];
            cov[c] = (float)s0;
            SUM[c] = s0 - rm1[c];
        }
        const float a = cov[0] * 0.5f, b = cov[1], cc = cov[2] * 0.5f;
        E[(long long)y * w + x] = (a + cc) - sqrtf((a - cc) * (a - cc) + b * b);
#pragma unroll
        for (int c = 0; c < 3; c++) { rm1[c] = r0[c]; r0[c] = rp1[c]; }
    }
}

// minMaxLoc(eig, 0, &maxVal, 0, 0, mask)
__global__ __launch_bounds__(256) void k_gftt_max(GfttArgs A, int pass)
{
    const int item = blockIdx.y;
    if (!g_active(A, item, pass)) return;
    const long long npx = (long long)A.w * A.h;
    const float *E = A.eig + item * A.px_stride;
    const uint8_t *M = A.mask + item * A.mask_stride;
    unsigned best = 0u;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < npx; p += (long long)gridDim.x * 256)
        if (M[p]) best = max(best, g_ord(E[p]));
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) best = max(best, (unsigned)__shfl_xor((int)best, off, 64));
    if ((threadIdx.x & 63) == 0 && best) atomicMax(&A.it[item].maxbits[pass], best);
}

// candidates per interior row: one wavefront per row
__global__ __launch_bounds__(256) void k_gftt_rows(GfttArgs A, int pass)
{
    const int item = blockIdx.y, y = blockIdx.x * 4 + (threadIdx.x >> 6) + 1, lane = threadIdx.x & 63;
    if (!g_active(A, item, pass) || y > A.h - 2) return;
    const float thr = g_thresh(A, item, pass);
    const float *E = A.eig + item * A.px_stride;
    const uint8_t *M = A.mask + item * A.mask_stride;
    int cnt = 0;
    for (int x0 = 1; x0 <= A.w - 2; x0 += 64) {
        const int x = x0 + lane;
        float v;
        const bool c = x <= A.w - 2 && g_is_cand(E, M, A.w, x, y, thr, &v);
        cnt += __popcll(__builtin_amdgcn_ballot_w64(c));
    }
    if (lane == 0) A.rowcnt[(long long)item * A.row_stride + y] = cnt;
}

// exclusive scan over the rows in DESCENDING order (row h-2 first): rowcnt[y] becomes the row's first slot
__global__ __launch_bounds__(1024) void k_gftt_scan(GfttArgs A, int pass)
{
    const int item = blockIdx.x, t = threadIdx.x;
    if (!g_active(A, item, pass)) return;
    __shared__ int part[1024];
    int *rc = A.rowcnt + (long long)item * A.row_stride;
    const int R = A.h - 2;                 // rows 1 .. h-2, j = 0 .. R-1 is row h-2-j
    const int per = R > 0 ? (R + 1023) / 1024 : 0;
    int s = 0;
    for (int j = t * per; j < min(R, (t + 1) * per); j++) s += rc[A.h - 2 - j];
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - s;
    for (int j = t * per; j < min(R, (t + 1) * per); j++) {
        const int y = A.h - 2 - j, c = rc[y];
        rc[y] = run; run += c;
    }
    if (t == 1023) A.it[item].ncand = part[1023];
    if (t == 0) A.it[item].sorted_b = 0;
}

// the candidates of a row at its slot, x descending: key ~ord(value) (ascending key = descending value), offset y*w + x
__global__ __launch_bounds__(256) void k_gftt_write(GfttArgs A, int pass)
{
    const int item = blockIdx.y, y = blockIdx.x * 4 + (threadIdx.x >> 6) + 1, lane = threadIdx.x & 63;
    if (!g_active(A, item, pass) || y > A.h - 2) return;
    const float thr = g_thresh(A, item, pass);
    const float *E = A.eig + item * A.px_stride;
    const uint8_t *M = A.mask + item * A.mask_stride;
    unsigned *K = A.keyA + item * A.cand_stride, *V = A.valA + item * A.cand_stride;
    int pos = A.rowcnt[(long long)item * A.row_stride + y];
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int xs = A.w - 2; xs >= 1; xs -= 64) {
        const int x = xs - lane;
        float v = 0.f;
        const bool c = x >= 1 && g_is_cand(E, M, A.w, x, y, thr, &v);
        const unsigned long long b = __builtin_amdgcn_ballot_w64(c);
        if (c) {
            const int at = pos + __popcll(b & lt);
            K[at] = ~g_ord(v); V[at] = (unsigned)(y * A.w + x);
        }
        pos += __popcll(b);
    }
}

// stable LSD radix sort of (key, offset) by key, 8-bit digits, one work-group per item; a pass whose digit is the same for every
// key is skipped.  Result in A or B (it[item].sorted_b).
__global__ __launch_bounds__(1024) void k_gftt_sort(GfttArgs A, int pass)
{
    const int item = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    if (!g_active(A, item, pass)) return;
    const int n = A.it[item].ncand;
    if (n <= 1) return;
    __shared__ int hist[256], base[256], scan_tmp[256];
    __shared__ int wcnt[16][256];
    __shared__ int skip;
    unsigned *K0 = A.keyA + item * A.cand_stride, *V0 = A.valA + item * A.cand_stride;
    unsigned *K1 = A.keyB + item * A.cand_stride, *V1 = A.valB + item * A.cand_stride;
    const unsigned long long lt = (1ull << lane) - 1ull;
    int inb = 0;
    for (int shift = 0; shift < 32; shift += 8) {
        const unsigned *Ks = inb ? K1 : K0, *Vs = inb ? V1 : V0;
        unsigned *Kd = inb ? K0 : K1, *Vd = inb ? V0 : V1;
        if (t < 256) hist[t] = 0;
        if (t == 0) skip = 0;
        __syncthreads();
        for (int i = t; i < n; i += 1024) atomicAdd(&hist[(Ks[i] >> shift) & 255u], 1);
        __syncthreads();
        if (t < 256) { scan_tmp[t] = hist[t]; if (hist[t] == n) skip = 1; }
        __syncthreads();
        if (skip) { __syncthreads(); continue; }
        for (int off = 1; off < 256; off <<= 1) {
            const int v = (t < 256 && t >= off) ? scan_tmp[t - off] : 0;
            __syncthreads();
            if (t < 256) scan_tmp[t] += v;
            __syncthreads();
        }
        if (t < 256) base[t] = scan_tmp[t] - hist[t];
        __syncthreads();
        for (int t0 = 0; t0 < n; t0 += 1024) {
            for (int k = t; k < 16 * 256; k += 1024) (&wcnt[0][0])[k] = 0;
            __syncthreads();
            const int i = t0 + t;
            const bool valid = i < n;
            const unsigned key = valid ? Ks[i] : 0u, val = valid ? Vs[i] : 0u;
            const int d = (int)((key >> shift) & 255u);
            unsigned long long m = __builtin_amdgcn_ballot_w64(valid);
#pragma unroll
            for (int b = 0; b < 8; b++) {
                const unsigned long long bb = __builtin_amdgcn_ballot_w64(valid && ((d >> b) & 1));
                m &= ((d >> b) & 1) ? bb : ~bb;
            }
            const int rank = __popcll(m & lt);
            if (valid && rank == 0) wcnt[wv][d] = __popcll(m);
            __syncthreads();
            if (t < 256) {
                int run = base[t];
#pragma unroll
                for (int k = 0; k < 16; k++) { const int c = wcnt[k][t]; wcnt[k][t] = run; run += c; }
                base[t] = run;
            }
            __syncthreads();
            if (valid) { const int at = wcnt[wv][d] + rank; Kd[at] = key; Vd[at] = val; }
            __syncthreads();
        }
        inb ^= 1;
    }
    if (t == 0) A.it[item].sorted_b = inb;
}

// greedy minimum-distance selection in sorted order (featureselect.cpp: a candidate is rejected when an accepted point lies at
// dx^2 + dy^2 < minDistance^2 -- such a point is always in the 3x3 neighbouring cells of OpenCV's grid, so the test is global);
// stops at maxCorners.  One wavefront per item; LDS: heads[cells] (int16), pts[cap] (x | y << 16), next[cap] (int16).
__global__ __launch_bounds__(64) void k_gftt_walk(GfttArgs A, int pass, int G, int gw, int gh, int cap)
{
    extern __shared__ unsigned char g_lds[];
    const int item = blockIdx.x, lane = threadIdx.x;
    if (!g_active(A, item, pass)) return;
    GfttItem &I = A.it[item];
    const int md = pass == 0 ? A.nmaxdist : A.nmindist, md2 = md * md;
    const int maxc = pass == 0 ? I.nb2d : I.nb2d - I.n1;
    short *heads = (short *)g_lds;
    unsigned *pts = (unsigned *)(g_lds + (((size_t)gw * gh * 2 + 15) & ~(size_t)15));
    short *nxt = (short *)(pts + cap);
    for (int k = lane; k < gw * gh; k += 64) heads[k] = -1;
    __syncthreads();
    const int n = I.ncand;
    const unsigned *V = (I.sorted_b ? A.valB : A.valA) + item * A.cand_stride;
    float2 *out = (pass == 0 ? A.out : A.out2) + (long long)item * A.out_cap;
    int count = 0;
    for (int b0 = 0; b0 < n && count < maxc; b0 += 64) {
        const int i = b0 + lane;
        const bool valid = i < n;
        const unsigned off = valid ? V[i] : 0u;
        const int y = (int)(off / (unsigned)A.w), x = (int)(off - (unsigned)y * (unsigned)A.w);
        bool good = valid;
        if (good) {
            const int gx = x / G, gy = y / G;
            for (int yy = max(gy - 1, 0); yy <= min(gy + 1, gh - 1) && good; yy++)
                for (int xx = max(gx - 1, 0); xx <= min(gx + 1, gw - 1) && good; xx++)
                    for (int j = heads[yy * gw + xx]; j >= 0; j = nxt[j]) {
                        const unsigned p = pts[j];
                        const int ddx = x - (int)(p & 0xffffu), ddy = y - (int)(p >> 16);
                        if (ddx * ddx + ddy * ddy < md2) { good = false; break; }
                    }
        }
        unsigned long long pend = __builtin_amdgcn_ballot_w64(good);
        while (pend && count < maxc) {
            const int l = __builtin_ctzll(pend);
            const int xl = __builtin_amdgcn_readlane(x, l), yl = __builtin_amdgcn_readlane(y, l);
            if (lane == 0) {
                const int cell = (yl / G) * gw + xl / G;
                pts[count] = (unsigned)xl | ((unsigned)yl << 16);
                nxt[count] = heads[cell];
                heads[cell] = (short)count;
                out[count] = make_float2((float)xl, (float)yl);
            }
            count++;
            if (good && lane > l) {
                const int ddx = x - xl, ddy = y - yl;
                if (ddx * ddx + ddy * ddy < md2) good = false;
            }
            pend = __builtin_amdgcn_ballot_w64(good && lane > l);
        }
        __syncthreads();
    }
    if (lane == 0) {
        if (pass == 0) {
            I.n1 = count;
            I.pass2 = !((double)count >= 0.66 * (double)I.nb2d || I.nb2d < 20);     // :160-163
        } else {
            I.n2 = count;
        }
    }
}

// pass-2 points after the pass-1 points (:208-211)
__global__ __launch_bounds__(64) void k_gftt_append(GfttArgs A, int *total)
{
    const int item = blockIdx.x;
    const GfttItem &I = A.it[item];
    const int n1 = I.nb2d > 0 ? I.n1 : 0, n2 = I.nb2d > 0 && I.pass2 ? I.n2 : 0;
    float2 *out = A.out + (long long)item * A.out_cap;
    const float2 *o2 = A.out2 + (long long)item * A.out_cap;
    for (int k = threadIdx.x; k < n2; k += 64) out[n1 + k] = o2[k];
    if (threadIdx.x == 0) total[item] = n1 + n2;
}

// ---------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------
static inline size_t g_up(size_t v) { return (v + 255) & ~(size_t)255; }

// per-item scratch of a chunk
static size_t gftt_item_bytes(int w, int h, int out_cap)
{
    const size_t npx = (size_t)w * h, nc = (size_t)(w - 2) * (h - 2);
    return g_up(4 * npx) + g_up(npx) + 4 * g_up(4 * nc) + g_up(4 * (size_t)h) + g_up(8 * (size_t)out_cap) + g_up(sizeof(GfttItem));
}

static int gftt_check_params(const ov2_gftt_params *p)
{
    OV2_REQUIRE(p != nullptr, OV2_EINVAL, "params == NULL");
    OV2_REQUIRE(p->nmaxdist >= 0 && p->nmindist >= 0, OV2_EINVAL, "negative keypoint distance");
    OV2_REQUIRE(p->nmaxdist <= GFTT_MAX_RADIUS && p->nmindist <= GFTT_MAX_RADIUS, OV2_EUNSUPPORTED, "keypoint distance above 63");
    OV2_REQUIRE(p->dminquality > 0.0 && p->dmaxquality > 0.0, OV2_EINVAL, "quality must be > 0 (goodFeaturesToTrack asserts it)");
    return OV2_OK;
}

// upper bound of nb2detect over the items (host-known part of it)
static int gftt_nb2d_bound(const ov2_gftt_params *p, int nbmax) { return nbmax == -1 ? std::max(p->nmaxpts, 0) : nbmax; }

// Enqueue detectGFTT for `items` device images; everything addressed from the context's scratch at `scratch` (which the caller has
// reserved: gftt_scratch_bytes).  out_d: out_cap points per item; n_d: per-item counts.  Asynchronous on ctx->stream.
static size_t gftt_scratch_bytes(int w, int h, int out_cap, int items, int *chunk)
{
    const size_t per = gftt_item_bytes(w, h, out_cap);
    size_t c = GFTT_SCRATCH_BUDGET / per;
    if (c < 1) c = 1;
    if (c > (size_t)items) c = (size_t)items;
    if (c > 65535) c = 65535;
    *chunk = (int)c;
    return per * c;
}

static int gftt_enqueue(ov2_ctx *ctx, const uint8_t *img, int w, int h, int stride, long long img_item_stride, int items,
                        const uint8_t *roi_d, int roi_stride, const ov2_gftt_params *p, const float2 *cur_d, int cur_cap,
                        const int *ncur_d, int ncur_all, const int *nbmax_d, int nb2d_bound, int do_subpix,
                        float2 *out_d, int out_cap, int *n_d, uint8_t *scratch, int chunk)
{
    // walk geometry (same for every item and pass): cell side >= minDistance, at most GFTT_GRID_MAX cells
    int G[2], gw[2], gh[2];
    for (int ps = 0; ps < 2; ps++) {
        int g = std::max(ps == 0 ? p->nmaxdist : p->nmindist, 1);
        while ((long long)((w + g - 1) / g) * ((h + g - 1) / g) > GFTT_GRID_MAX) g++;
        G[ps] = g; gw[ps] = (w + g - 1) / g; gh[ps] = (h + g - 1) / g;
    }
    const int cap = std::max(nb2d_bound, 1);
    const size_t npx = (size_t)w * h, nc = (size_t)(w - 2) * (h - 2);
    GfttArgs A;
    memset(&A, 0, sizeof(A));
    A.w = w; A.h = h; A.stride = stride; A.img_item_stride = img_item_stride;
    A.roi = roi_d; A.roi_stride = roi_stride; A.cur_cap = cur_cap; A.ncur_all = ncur_all;
    A.nmaxpts = p->nmaxpts; A.nmaxdist = p->nmaxdist; A.nmindist = p->nmindist; A.q1 = p->dminquality; A.q2 = p->dmaxquality;
    A.sobel_dy_order = ctx->sobel_dy_order;
    A.px_stride = (long long)g_up(4 * npx) / 4; A.mask_stride = (long long)g_up(npx);
    A.cand_stride = (long long)g_up(4 * nc) / 4;
    A.row_stride = (int)(g_up(4 * (size_t)h) / 4);
    A.out_cap = out_cap;
    // chunk layout: [eig][mask][keyA][valA][keyB][valB][rows][out2][items]
    uint8_t *s = scratch;
    float *eig = (float *)s;                       s += (size_t)chunk * g_up(4 * npx);
    uint8_t *mask = s;                             s += (size_t)chunk * g_up(npx);
    unsigned *kA = (unsigned *)s;                  s += (size_t)chunk * g_up(4 * nc);
    unsigned *vA = (unsigned *)s;                  s += (size_t)chunk * g_up(4 * nc);
    unsigned *kB = (unsigned *)s;                  s += (size_t)chunk * g_up(4 * nc);
    unsigned *vB = (unsigned *)s;                  s += (size_t)chunk * g_up(4 * nc);
    int *rows = (int *)s;                          s += (size_t)chunk * g_up(4 * (size_t)h);
    float2 *out2 = (float2 *)s;                    s += (size_t)chunk * g_up(8 * (size_t)out_cap);
    GfttItem *it = (GfttItem *)s;
    A.eig = eig; A.mask = mask; A.keyA = kA; A.valA = vA; A.keyB = kB; A.valB = vB; A.rowcnt = rows; A.out2 = out2; A.it = it;
    const size_t walk_lds0 = (((size_t)gw[0] * gh[0] * 2 + 15) & ~(size_t)15) + (size_t)cap * 6;
    const size_t walk_lds1 = (((size_t)gw[1] * gh[1] * 2 + 15) & ~(size_t)15) + (size_t)cap * 6;
    const int px_blocks = (int)std::min<size_t>((npx + 255) / 256, 1024);
    const int row_blocks = (h - 2 + 3) / 4;
    for (int c0 = 0; c0 < items; c0 += chunk) {
        const int n = std::min(chunk, items - c0);
        A.img = img + (long long)c0 * img_item_stride;
        A.cur = cur_d ? cur_d + (long long)c0 * cur_cap : nullptr;
        A.ncur = ncur_d ? ncur_d + c0 : nullptr;
        A.nbmax = nbmax_d + c0;
        A.out = out_d + (long long)c0 * out_cap;
        const int ncirc0 = cur_d ? cur_cap : 0;
        hipLaunchKernelGGL(k_gftt_setup, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, A, n);
        hipLaunchKernelGGL(k_gftt_eig, dim3((w + 63) / 64, n), dim3(64), 0, ctx->stream, A);
        for (int ps = 0; ps < 2; ps++) {
            hipLaunchKernelGGL(k_gftt_mask_init, dim3(px_blocks, n), dim3(256), 0, ctx->stream, A, ps);
            const int ncirc = ncirc0 + (ps == 1 ? out_cap : 0);
            if (ncirc > 0) hipLaunchKernelGGL(k_gftt_circles, dim3(ncirc, n), dim3(64), 0, ctx->stream, A, ps);
            hipLaunchKernelGGL(k_gftt_max, dim3(px_blocks, n), dim3(256), 0, ctx->stream, A, ps);
            hipLaunchKernelGGL(k_gftt_rows, dim3(row_blocks, n), dim3(256), 0, ctx->stream, A, ps);
            hipLaunchKernelGGL(k_gftt_scan, dim3(n), dim3(1024), 0, ctx->stream, A, ps);
            hipLaunchKernelGGL(k_gftt_write, dim3(row_blocks, n), dim3(256), 0, ctx->stream, A, ps);
            hipLaunchKernelGGL(k_gftt_sort, dim3(n), dim3(1024), 0, ctx->stream, A, ps);
            hipLaunchKernelGGL(k_gftt_walk, dim3(n), dim3(64), ps == 0 ? walk_lds0 : walk_lds1, ctx->stream, A, ps, G[ps], gw[ps], gh[ps], cap);
            OV2_HIP_CHECK(hipGetLastError());
            if (do_subpix) {
                const int rc = launch_subpix(ctx->stream, A.img, w, h, stride, ps == 0 ? A.out : A.out2, out_cap, 3, 30, 0.01,
                                             ps == 0 ? &it[0].n1 : &it[0].n2, n, img_item_stride, out_cap, (int)(sizeof(GfttItem) / sizeof(int)));
                if (rc) return rc;
            }
        }
        hipLaunchKernelGGL(k_gftt_append, dim3(n), dim3(64), 0, ctx->stream, A, n_d + c0);
        OV2_HIP_CHECK(hipGetLastError());
    }
    return OV2_OK;
}

static int gftt_check_geometry(int w, int h, int stride)
{
    OV2_REQUIRE(stride >= w, OV2_EINVAL, "stride < width");
    OV2_REQUIRE(w >= 16 && h >= 16, OV2_EUNSUPPORTED, "image smaller than 16 x 16");
    OV2_REQUIRE(w < 65536 && h < 65536 && (long long)w * h < (1ll << 31), OV2_EUNSUPPORTED, "image too large");
    return OV2_OK;
}

// one image: img_h (uploaded) or img_d (device, no upload); host roi / keypoints / output; one synchronisation
static int gftt_single(ov2_ctx *ctx, const uint8_t *img_h, const uint8_t *img_d, int w, int h, int stride, const uint8_t *roi_h,
                       int roi_stride, const ov2_gftt_params *p, const float *cur_xy_h, int ncur, int nbmax, int do_subpix,
                       float *out_xy_h, int out_cap, int *out_n)
{
    OV2_REQUIRE(ctx && out_n, OV2_EINVAL, "NULL argument");
    *out_n = 0;
    int rc = gftt_check_params(p); if (rc) return rc;
    OV2_REQUIRE(nbmax == -1 || nbmax >= 1, OV2_EINVAL, "nbmax must be -1 or >= 1");
    OV2_REQUIRE(ncur >= 0 && (ncur == 0 || cur_xy_h), OV2_EINVAL, "bad current keypoints");
    if ((!img_h && !img_d) || w <= 0 || h <= 0) return OV2_OK;            // empty image -> empty vector
    if (ncur >= p->nmaxpts) return OV2_OK;                                // :108-111
    const int nb2d = nbmax != -1 ? nbmax : p->nmaxpts - ncur;
    OV2_REQUIRE(out_xy_h && out_cap >= nb2d, OV2_EINVAL, "out_cap below nb2detect");
    OV2_REQUIRE(nb2d <= GFTT_MAX_CORNERS, OV2_EUNSUPPORTED, "nb2detect above 4096");
    rc = gftt_check_geometry(w, h, stride); if (rc) return rc;
    OV2_REQUIRE(!roi_h || roi_stride >= w, OV2_EINVAL, "roi stride < width");
    OV2_HIP_CHECK(hipSetDevice(ctx->device));
    const int cap = nb2d;
    int chunk;
    const size_t work = gftt_scratch_bytes(w, h, cap, 1, &chunk);
    // device scratch: [work][image][roi][cur][nbmax][out][count]
    const size_t o_img = g_up(work);
    const size_t o_roi = o_img + (img_d ? 0 : g_up((size_t)w * h));
    const size_t o_cur = o_roi + (roi_h ? g_up((size_t)w * h) : 0);
    const size_t o_nb = o_cur + g_up(8 * (size_t)std::max(ncur, 1));
    const size_t o_out = o_nb + 256;
    const size_t o_n = o_out + 8 * (size_t)cap;
    rc = ctx->reserve_device(o_n + 16); if (rc) return rc;
    rc = ctx->reserve_host(8 * (size_t)cap + 16); if (rc) return rc;
    uint8_t *ds = (uint8_t *)ctx->d_scratch;
    const uint8_t *im = img_d;
    int im_stride = stride;
    if (!img_d) {
        rc = ctx->upload_image(ds + o_img, (size_t)w, img_h, (size_t)stride, (size_t)w, (size_t)h); if (rc) return rc;
        im = ds + o_img; im_stride = w;
    }
    if (roi_h) OV2_HIP_CHECK(hipMemcpy2DAsync(ds + o_roi, (size_t)w, roi_h, (size_t)roi_stride, (size_t)w, (size_t)h, hipMemcpyHostToDevice, ctx->stream));
    if (ncur > 0) OV2_HIP_CHECK(hipMemcpyAsync(ds + o_cur, cur_xy_h, 8 * (size_t)ncur, hipMemcpyHostToDevice, ctx->stream));
    int *hs = (int *)ctx->h_scratch;
    hs[0] = nbmax;
    OV2_HIP_CHECK(hipMemcpyAsync(ds + o_nb, hs, 4, hipMemcpyHostToDevice, ctx->stream));
    rc = gftt_enqueue(ctx, im, w, h, im_stride, 0, 1, roi_h ? ds + o_roi : nullptr, w, p, ncur > 0 ? (const float2 *)(ds + o_cur) : nullptr, ncur,
                      nullptr, ncur, (const int *)(ds + o_nb), nb2d, do_subpix, (float2 *)(ds + o_out), cap, (int *)(ds + o_n), ds, chunk);
    if (rc) return rc;
    OV2_HIP_CHECK(hipMemcpyAsync(hs, ds + o_out, 8 * (size_t)cap + 4, hipMemcpyDeviceToHost, ctx->stream));
    OV2_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    const int n = hs[2 * cap];
    if (n > 0) memcpy(out_xy_h, hs, 8 * (size_t)n);
    *out_n = n;
    return OV2_OK;
}

extern "C" {

int ov2_gftt_params_init(int nmaxpts, int nmaxdist, double dmaxquality, ov2_gftt_params *out)
{
    OV2_REQUIRE(out != nullptr, OV2_EINVAL, "out == NULL");
    OV2_REQUIRE(nmaxpts >= 0 && nmaxdist >= 0, OV2_EINVAL, "negative size");
    out->nmaxpts = nmaxpts; out->nmaxdist = nmaxdist;
    out->nmindist = nmaxdist / 2;                   // size_t = double: truncated (:81)
    out->dmaxquality = dmaxquality;
    out->dminquality = dmaxquality / 2.;            // :82
    return OV2_OK;
}

int ov2_detect_gftt(ov2_ctx *ctx, const uint8_t *img_h, int w, int h, int stride, const uint8_t *roi_h, int roi_stride,
                    const ov2_gftt_params *params, const float *cur_xy_h, int ncur, int nbmax, int do_subpix,
                    float *out_xy_h, int out_cap, int *out_n)
{
    return gftt_single(ctx, img_h, nullptr, w, h, stride, roi_h, roi_stride, params, cur_xy_h, ncur, nbmax, do_subpix, out_xy_h, out_cap, out_n);
}

int ov2_detect_gftt_d(ov2_ctx *ctx, const ov2_pyr *pyr, int item, const uint8_t *roi_h, int roi_stride,
                      const ov2_gftt_params *params, const float *cur_xy_h, int ncur, int nbmax, int do_subpix,
                      float *out_xy_h, int out_cap, int *out_n)
{
    OV2_REQUIRE(ctx && pyr && out_n, OV2_EINVAL, "NULL argument");
    *out_n = 0;
    OV2_REQUIRE(item >= 0 && item < pyr->d.batch, OV2_EINVAL, "batch item out of range");
    const PyrLevelDesc &L0 = pyr->d.lv[0];
    const uint8_t *img = pyr->d.base + (long long)item * pyr->d.item_stride + L0.img_roi;
    const int rc = ov2_pyr_wait_ready(ctx, pyr);
    if (rc != OV2_OK) return rc;
    return gftt_single(ctx, nullptr, img, L0.w, L0.h, L0.img_pitch, roi_h, roi_stride, params, cur_xy_h, ncur, nbmax, do_subpix, out_xy_h, out_cap, out_n);
}

int ov2_detect_gftt_batch_d(ov2_ctx *ctx, const ov2_pyr *pyr, const uint8_t *roi_d, int roi_stride, const ov2_gftt_params *params,
                            const float *cur_xy_d, int cur_cap, const int *ncur_d, const int *nbmax_h, int do_subpix,
                            float *out_xy_d, int out_cap, int *out_n_h)
{
    OV2_REQUIRE(ctx && pyr && nbmax_h && out_xy_d && out_n_h, OV2_EINVAL, "NULL argument");
    int rc = gftt_check_params(params); if (rc) return rc;
    const int items = pyr->d.batch;
    const PyrLevelDesc &L0 = pyr->d.lv[0];
    const int w = L0.w, h = L0.h;
    OV2_REQUIRE(cur_cap >= 0 && (ncur_d == nullptr || cur_xy_d != nullptr), OV2_EINVAL, "bad current keypoints");
    OV2_REQUIRE(!roi_d || roi_stride >= w, OV2_EINVAL, "roi stride < width");
    int bound = 0;
    for (int i = 0; i < items; i++) {
        out_n_h[i] = 0;
        OV2_REQUIRE(nbmax_h[i] == -1 || nbmax_h[i] >= 1, OV2_EINVAL, "nbmax must be -1 or >= 1");
        bound = std::max(bound, gftt_nb2d_bound(params, nbmax_h[i]));
    }
    OV2_REQUIRE(out_cap >= bound, OV2_EINVAL, "out_cap below nb2detect (nbmax, or nmaxpts where nbmax is -1)");
    OV2_REQUIRE(bound <= GFTT_MAX_CORNERS, OV2_EUNSUPPORTED, "nb2detect above 4096");
    if (w <= 0 || h <= 0 || items <= 0) return OV2_OK;
    rc = gftt_check_geometry(w, h, L0.img_pitch); if (rc) return rc;
    rc = ov2_pyr_wait_ready(ctx, pyr); if (rc) return rc;
    OV2_HIP_CHECK(hipSetDevice(ctx->device));
    int chunk;
    const size_t work = gftt_scratch_bytes(w, h, out_cap, items, &chunk);
    const size_t o_nb = g_up(work), o_n = o_nb + g_up(4 * (size_t)items);
    rc = ctx->reserve_device(o_n + 4 * (size_t)items); if (rc) return rc;
    rc = ctx->reserve_host(4 * (size_t)items); if (rc) return rc;
    uint8_t *ds = (uint8_t *)ctx->d_scratch;
    int *hs = (int *)ctx->h_scratch;
    memcpy(hs, nbmax_h, 4 * (size_t)items);
    OV2_HIP_CHECK(hipMemcpyAsync(ds + o_nb, hs, 4 * (size_t)items, hipMemcpyHostToDevice, ctx->stream));
    const uint8_t *img = pyr->d.base + L0.img_roi;
    rc = gftt_enqueue(ctx, img, w, h, L0.img_pitch, (long long)pyr->d.item_stride, items, roi_d, roi_stride, params,
                      ncur_d ? (const float2 *)cur_xy_d : nullptr, cur_cap, ncur_d, 0, (const int *)(ds + o_nb), bound, do_subpix,
                      (float2 *)out_xy_d, out_cap, (int *)(ds + o_n), ds, chunk);
    if (rc) return rc;
    OV2_HIP_CHECK(hipMemcpyAsync(hs, ds + o_n, 4 * (size_t)items, hipMemcpyDeviceToHost, ctx->stream));
    OV2_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    memcpy(out_n_h, hs, 4 * (size_t)items);
    return OV2_OK;
}

// FeatureExtractor::setMask on a host mask: a filled disc of radius `dist` (value 0) at cvRound of every point
int ov2_set_mask(uint8_t *mask, int w, int h, int stride, const float *xy, int n, int dist)
{
    OV2_REQUIRE(mask && w > 0 && h > 0 && stride >= w, OV2_EINVAL, "bad mask");
    OV2_REQUIRE(n >= 0 && (n == 0 || xy), OV2_EINVAL, "bad points");
    OV2_REQUIRE(dist >= 0, OV2_EINVAL, "negative radius");
    for (int i = 0; i < n; i++) {
        const float fx = xy[2 * i], fy = xy[2 * i + 1];
        if (!(fabsf(fx) < 1e7f && fabsf(fy) < 1e7f)) continue;
        const int cx = (int)rintf(fx), cy = (int)rintf(fy);
        // drawing.cpp Circle(), fill variant: every hline of a step is centred on cx, so a row's span is its widest one
        int err = 0, dx = dist, dy = 0, plus = 1, minus = (dist << 1) - 1;
        auto hline = [&](int y, int x0, int x1) {
            if (y < 0 || y >= h) return;
            x0 = std::max(x0, 0); x1 = std::min(x1, w - 1);
            if (x0 <= x1) memset(mask + (size_t)y * stride + x0, 0, (size_t)(x1 - x0 + 1));
        };
        while (dx >= dy) {
            hline(cy - dy, cx - dx, cx + dx); hline(cy + dy, cx - dx, cx + dx);
            hline(cy - dx, cx - dy, cx + dy); hline(cy + dx, cx - dy, cx + dy);
            dy++; err += plus; plus += 2;
            const int m = (err <= 0) - 1;
            err -= minus & m; dx += m; minus -= m & 2;
        }
    }
    return OV2_OK;
}

} // extern "C"
