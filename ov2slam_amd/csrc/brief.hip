// brief.hip -- FeatureExtractor::describeBRIEF (/root/reference/src/feature_extractor.cpp:224-285): OpenCV contrib's
// BriefDescriptorExtractor with its defaults (32 bytes, no orientation) on a device image, bit-exact (DESIGN.md "BRIEF").
//
// Semantics (restated from the public OpenCV source, brief.cpp / keypoint.cpp; to be confirmed on a real OpenCV build):
//   keep     28 <= rint(x) < W-28 and 28 <= rint(y) < H-28 (runByImageBorder: Point2f -> Point rounds half to even)
//   centre   cx = (int)(x + 0.5), cy = (int)(y + 0.5)  (double in OpenCV; floorf(x + 0.5f) is the same integer for every float
//            that passes the border rule in an image narrower than 2^20 -- tests/test_brief_reference.py checks [27.5, 4096))
//   S(dy,dx) the sum of the 9x9 pixels centred at (cy+dy, cx+dx); bit t = S(ay,ax) < S(by,bx); byte j = bits 8j..8j+7, MSB first
// One exception: odd W, x == W-28.5 and a +24 column offset (rows alike) put a box one column past the image, where OpenCV reads
// past its integral image's row.  Here every pixel outside the image counts 0: the sum over the box's in-image pixels.
//
// Kernel k_brief32: one wavefront per keypoint, four per work-group.  The 57x57 patch [-28, 28]^2 around the centre is read one
// row per load instruction (lane = column) and turned into its 58x58 integral image in LDS: a running column sum in registers, then
// one row prefix per lane.  The table is kept modulo 2^16 (6.7 KB per wavefront): a 9x9 box sum is at most 81*255 < 2^16, so the
// four-term difference taken modulo 2^16 IS the box sum.  Lane l evaluates tests 64k + (l ^ 7), k = 0..3: the four ballots are
// the descriptor's bytes in order, MSB first, with no bit reversal.
#include "common.hpp"
#include "brief_pattern.hpp"

#define BRIEF_BORDER 28            // PATCH_SIZE/2 + KERNEL_SIZE/2
#define BRIEF_P 57                 // patch side: offsets [-24, 24] plus the box half-width 4
#define BRIEF_T 58                 // integral table side (row and column 0 are zero); 29 dwords per row: odd, no bank conflicts
#define BRIEF_WAVES 4              // keypoints per work-group
#define BRIEF_MAX_SIDE (1 << 20)   // floorf(x + 0.5f) == (int)((double)x + 0.5) for every surviving x below this

__global__ __launch_bounds__(64 * BRIEF_WAVES)
void k_brief32(const uint8_t *__restrict__ img, int w, int h, long long pitch, long long item_stride,
               const float *__restrict__ xy, int cap, const int *__restrict__ n_d, int n_all,
               const int *__restrict__ pat, uint8_t *__restrict__ desc, uint8_t *__restrict__ valid)
{
    __shared__ uint16_t tab[BRIEF_WAVES][BRIEF_T * BRIEF_T];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int item = blockIdx.y;
    const int i = blockIdx.x * BRIEF_WAVES + wv;
    int n = n_d ? n_d[item] : n_all;
    n = n < cap ? n : cap;
    const bool in = i < n;
    const long long slot = (long long)item * cap + i;
    bool ok = false;
    int cx = 0, cy = 0;
    if (in) {
        const float x = xy[2 * slot], y = xy[2 * slot + 1];
        const float rx = rintf(x), ry = rintf(y);         // NaN and +-inf fail every comparison below
        ok = rx >= (float)BRIEF_BORDER && rx < (float)(w - BRIEF_BORDER) && ry >= (float)BRIEF_BORDER && ry < (float)(h - BRIEF_BORDER);
        if (ok) { cx = (int)floorf(x + 0.5f); cy = (int)floorf(y + 0.5f); }
    }
    uint16_t *T = tab[wv];
    // column sums: lane c walks column cx-28+c downwards; pixels outside the image (column W / row H in the odd-size case) are 0
    if (ok && lane < BRIEF_P) {
        const int gx = cx - BRIEF_BORDER + lane;
        const bool colin = (unsigned)gx < (unsigned)w;
        const uint8_t *src = img + (long long)item * item_stride + gx;
        uint32_t v[BRIEF_P];
#pragma unroll
        for (int r = 0; r < BRIEF_P; r++) {
            const int gy = cy - BRIEF_BORDER + r;
            v[r] = colin && (unsigned)gy < (unsigned)h ? src[(long long)gy * pitch] : 0u;
        }
        uint32_t acc = 0;
        T[lane + 1] = 0;
#pragma unroll
        for (int r = 0; r < BRIEF_P; r++) { acc += v[r]; T[(r + 1) * BRIEF_T + lane + 1] = (uint16_t)acc; }
    }
    __syncthreads();
    // row prefixes: lane r turns row r of column sums into row r of the integral image (values wrap modulo 2^16 on purpose)
    if (ok && lane < BRIEF_T) {
        uint16_t *row = T + lane * BRIEF_T;
        uint32_t c[BRIEF_P];
#pragma unroll
        for (int k = 0; k < BRIEF_P; k++) c[k] = row[k + 1];
        uint32_t acc = 0;
        row[0] = 0;
#pragma unroll
        for (int k = 0; k < BRIEF_P; k++) { acc += c[k]; row[k + 1] = (uint16_t)acc; }
    }
    __syncthreads();
    if (!in) return;
    uint8_t *d = desc + slot * 32;
    if (!ok) {
        if (lane < 32) d[lane] = 0;
        if (lane == 0) valid[slot] = 0;
        return;
    }
    auto box = [&](int r, int c) -> uint32_t {       // r, c: top-left corner in the patch (offset + 24)
        const uint16_t *a = T + r * BRIEF_T + c, *b = a + 9 * BRIEF_T;
        return (uint32_t)(b[9] - a[9] - b[0] + a[0]) & 0xffffu;
    };
    unsigned long long bal[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int p = pat[64 * k + (lane ^ 7)];
        const int ay = (int8_t)(p & 0xff), ax = (int8_t)((p >> 8) & 0xff), by = (int8_t)((p >> 16) & 0xff), bx = (int8_t)(p >> 24);
        const bool bit = box(ay + 24, ax + 24) < box(by + 24, bx + 24);
        bal[k] = __ballot(bit);
    }
    if (lane < 32) d[lane] = (uint8_t)(bal[lane >> 3] >> (8 * (lane & 7)));
    if (lane == 0) valid[slot] = 1;
}

static int brief_check_pattern(const int8_t *pairs)
{
    for (int i = 0; i < 256 * 4; i++)
        if (pairs[i] < -24 || pairs[i] > 24) {
            ov2_set_error("BRIEF pattern entry %d (pair %d) is %d: offsets must lie in [-24, 24]", i, i / 4, (int)pairs[i]);
            return OV2_EINVAL;
        }
    return OV2_OK;
}

// the 1 KB device copy of the context's pattern, uploaded on the stream when it changed
static int brief_pattern_d(ov2_ctx *ctx, const int **out)
{
    if (!ctx->brief_pat_d) { OV2_HIP_CHECK(hipMalloc(&ctx->brief_pat_d, 256 * 4)); ctx->brief_pat_current = false; }
    if (!ctx->brief_pat_current) {
        // every describe entry point synchronises before it returns, so no earlier kernel still reads the buffer
        OV2_HIP_CHECK(hipMemcpyAsync(ctx->brief_pat_d, ctx->brief_custom ? ctx->brief_pat : OV2_BRIEF_DEFAULT_PATTERN, 256 * 4,
                                     hipMemcpyHostToDevice, ctx->stream));
        OV2_HIP_CHECK(hipStreamSynchronize(ctx->stream));      // the source may change with the next ov2_brief_set_pattern
        ctx->brief_pat_current = true;
    }
    *out = (const int *)ctx->brief_pat_d;
    return OV2_OK;
}

int ov2_brief_launch_d(ov2_ctx *ctx, const uint8_t *img_d, int w, int h, size_t pitch, size_t item_stride, int n_items,
                       const float *xy_d, int cap, const int *n_d, int n_all, uint8_t *desc_d, uint8_t *valid_d)
{
    const int *pat = nullptr;
    int rc = brief_pattern_d(ctx, &pat);
    if (rc != OV2_OK) return rc;
    hipLaunchKernelGGL(k_brief32, dim3((unsigned)((cap + BRIEF_WAVES - 1) / BRIEF_WAVES), (unsigned)n_items), dim3(64 * BRIEF_WAVES), 0,
                       ctx->stream, img_d, w, h, (long long)pitch, (long long)item_stride, xy_d, cap, n_d, n_all, pat, desc_d, valid_d);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

static int brief_check_geometry(int w, int h, size_t pitch, int n_items, int cap)
{
    OV2_REQUIRE(w > 0 && h > 0 && w < BRIEF_MAX_SIDE && h < BRIEF_MAX_SIDE, OV2_EINVAL, "image size out of range (1 .. 2^20 - 1)");
    OV2_REQUIRE(pitch >= (size_t)w, OV2_EINVAL, "stride < width");
    OV2_REQUIRE(n_items >= 1 && n_items <= 65535, OV2_EINVAL, "n_items out of range (1 .. 65535)");
    OV2_REQUIRE(cap >= 0 && cap <= (1 << 28), OV2_EINVAL, "point capacity out of range");
    return OV2_OK;
}


int ov2_brief_run_h(ov2_ctx *ctx, const uint8_t *img_h, const uint8_t *img_d, int w, int h, size_t pitch, size_t item_stride, int n_items,
                    const float *xy_h, const int *n_h, int n_h_all, int cap, uint8_t *desc_h, uint8_t *valid_h)
{
    int rc = brief_check_geometry(w, h, pitch, n_items, cap);
    if (rc != OV2_OK) return rc;
    int total = 0;
    for (int b = 0; b < n_items; b++) {
        const int n = n_h ? n_h[b] : n_h_all;
        OV2_REQUIRE(n >= 0 && n <= cap, OV2_EINVAL, "an item carries more points than the cap slots");
        total += n;
    }
    if (total == 0) return OV2_OK;
    OV2_REQUIRE(xy_h && desc_h && valid_h, OV2_EINVAL, "NULL point or result buffer");
    OV2_HIP_CHECK(hipSetDevice(ctx->device));
    // block (same layout on both sides): counts | points | descriptors | valid flags; the host image (if any) ahead of it on the device
    const size_t slots = (size_t)n_items * (size_t)cap;
    const size_t o_n = 0, o_xy = up256(4 * (size_t)n_items), o_desc = up256(o_xy + 8 * slots), o_valid = o_desc + 32 * slots;
    const size_t blk = up256(o_valid + slots);
    const size_t img_pitch = up256((size_t)w), img_bytes = img_h ? up256(img_pitch * (size_t)h) : 0;
    rc = ctx->reserve_host(blk);               if (rc != OV2_OK) return rc;
    rc = ctx->reserve_device(img_bytes + blk); if (rc != OV2_OK) return rc;
    uint8_t *dimg = (uint8_t *)ctx->d_scratch, *dblk = dimg + img_bytes, *hblk = (uint8_t *)ctx->h_scratch;
    if (img_h) {
        rc = ctx->upload_image(dimg, img_pitch, img_h, pitch, (size_t)w, (size_t)h);
        if (rc != OV2_OK) return rc;
        img_d = dimg; pitch = img_pitch; item_stride = img_bytes;
    }
    int *nn = (int *)(hblk + o_n);
    for (int b = 0; b < n_items; b++) {
        nn[b] = n_h ? n_h[b] : n_h_all;
        memcpy(hblk + o_xy + 8 * (size_t)b * cap, xy_h + 2 * (size_t)b * cap, 8 * (size_t)nn[b]);
    }
    OV2_HIP_CHECK(hipMemcpyAsync(dblk, hblk, o_desc, hipMemcpyHostToDevice, ctx->stream));
    rc = ov2_brief_launch_d(ctx, img_d, w, h, pitch, item_stride, n_items, (const float *)(dblk + o_xy), cap, (const int *)(dblk + o_n), 0,
                      dblk + o_desc, dblk + o_valid);
    if (rc != OV2_OK) return rc;
    OV2_HIP_CHECK(hipMemcpyAsync(hblk + o_desc, dblk + o_desc, blk - o_desc, hipMemcpyDeviceToHost, ctx->stream));
    OV2_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (int b = 0; b < n_items; b++) {
        const size_t o = (size_t)b * cap, n = (size_t)nn[b];
        memcpy(desc_h + 32 * o, hblk + o_desc + 32 * o, 32 * n);
        memcpy(valid_h + o, hblk + o_valid + o, n);
    }
    return OV2_OK;
}

extern "C" {

int ov2_brief_set_pattern(ov2_ctx *ctx, const int8_t *pairs)
{
    OV2_REQUIRE(ctx != nullptr, OV2_EINVAL, "ctx == NULL");
    if (!pairs) { ctx->brief_custom = false; ctx->brief_pat_current = false; return OV2_OK; }
    const int rc = brief_check_pattern(pairs);
    if (rc != OV2_OK) return rc;                     // the previous pattern stays
    memcpy(ctx->brief_pat, pairs, sizeof(ctx->brief_pat));
    ctx->brief_custom = true; ctx->brief_pat_current = false;
    return OV2_OK;
}

int ov2_brief_get_pattern(ov2_ctx *ctx, int8_t *pairs)
{
    OV2_REQUIRE(ctx != nullptr && pairs != nullptr, OV2_EINVAL, "NULL argument");
    memcpy(pairs, ctx->brief_custom ? ctx->brief_pat : OV2_BRIEF_DEFAULT_PATTERN, 256 * 4);
    return OV2_OK;
}

int ov2_describe_brief(ov2_ctx *ctx, const uint8_t *img_h, int w, int h, int stride, const float *xy_h, int n, uint8_t *desc_h, uint8_t *valid_h)
{
    OV2_REQUIRE(ctx != nullptr, OV2_EINVAL, "ctx == NULL");
    OV2_REQUIRE(n >= 0, OV2_EINVAL, "negative keypoint count");
    if (n == 0) return OV2_OK;
    OV2_REQUIRE(img_h != nullptr && stride >= w, OV2_EINVAL, "NULL image or stride < width");
    return ov2_brief_run_h(ctx, img_h, nullptr, w, h, (size_t)stride, 0, 1, xy_h, nullptr, n, n, desc_h, valid_h);
}

int ov2_describe_brief_batch_d(ov2_ctx *ctx, const uint8_t *img_d, int w, int h, int pitch, size_t item_stride, int n_items,
                               const float *xy_d, int cap, const int *n_d, uint8_t *desc_d, uint8_t *valid_d)
{
    OV2_REQUIRE(ctx != nullptr, OV2_EINVAL, "ctx == NULL");
    int rc = brief_check_geometry(w, h, (size_t)(pitch > 0 ? pitch : 0), n_items, cap);
    if (rc != OV2_OK) return rc;
    OV2_REQUIRE(n_items == 1 || item_stride >= (size_t)pitch * (size_t)h, OV2_EINVAL, "item_stride smaller than one image");
    if (cap == 0) return OV2_OK;
    OV2_REQUIRE(img_d && xy_d && desc_d && valid_d, OV2_EINVAL, "NULL device buffer");
    OV2_HIP_CHECK(hipSetDevice(ctx->device));
    rc = ov2_brief_launch_d(ctx, img_d, w, h, (size_t)pitch, item_stride, n_items, xy_d, cap, n_d, cap, desc_d, valid_d);
    if (rc != OV2_OK) return rc;
    OV2_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return OV2_OK;
}

} // extern "C"
