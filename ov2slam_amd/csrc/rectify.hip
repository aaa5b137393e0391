// rectify.hip -- CameraCalibration::rectifyImage (the reference's src/camera_calibration.cpp:233-241): the
// cv::remap(img, rect, undist_map_x_, undist_map_y_, cv::INTER_LINEAR) the reference runs on every frame, left and right,
// before preprocessImage when bdo_undist / bdo_stereo_rect is set (src/ov2slam.cpp:239-265).  OpenCV's own C++ path of
// cv::remap for CV_8UC1 / INTER_LINEAR / BORDER_CONSTANT 0, RESTATED (include/ov2slam_hip.h; tests/remap_ref.py), not pinned
// against an OpenCV build.
//
// Both map forms the reference creates (CV_32FC1 pair, setUndistMap :92 / :97; CV_16SC2 + CV_16UC1, setUndistStereoMap :141 /
// :145) are normalised ONCE on the host, at ov2_rectmap_create, to one device representation -- per destination pixel
// (ix, iy) as two int16 in a dword and b * 32 + a in a uint16, rows padded to 4 entries -- so there is one kernel path.
//
// k_remap: the destination is walked in tiles of 128 x 8 pixels; a lane owns 4 consecutive pixels of a row and stores them as
// one dword (a wavefront row: 128 B).  Its 4 map entries are read once (one 16-byte + one 8-byte load), turned into 8 row-pair
// offsets and 16 weights that stay in registers, and reused for every batch item the work-group serves, 6 B of map per pixel
// amortised over the items.  The two taps of a source row are neighbouring bytes: they come in ONE 2-byte load (the gather is
// bound by the number of load instructions, not by bytes: DESIGN 4.13), so per item it is 8 gathers and one dword store per
// lane -- or 3: a lane whose 8 pairs lie within 8 columns of 3 consecutive source rows (the rule under a smooth map) reads those
// three 8-byte row segments instead and shifts its pairs out of them.  The pair's column is clamped into [0, w - 2] and its row
// into the image, and a tap outside the source has weight 0: every load is unconditional and in bounds, and the inlier,
// partly-outside and fully-outside branches of OpenCV are one expression.  No LDS staging of the source footprint.
#include "common.hpp"
#include <cmath>
#include <new>

#define RM_TX 32        // lanes along x per work-group: 4 destination pixels each
#define RM_TY 8         // destination rows per work-group
#define RM_ITEMS 16     // batch items per work-group (the map entries are read once per work-group)

struct RemapArgs {
    const uint32_t *ixy;      // (uint16)ix | (uint16)iy << 16, `mpitch` entries per row
    const uint16_t *ab;       // b * 32 + a
    int w, h, mpitch;
    const uint8_t *src; int src_pitch; long long src_item;
    uint8_t *dst; int dst_pitch; long long dst_item;
    int n_items, per_wg;      // work-group z serves items [z * per_wg, min(n_items, (z + 1) * per_wg))
    int dword_ok;             // dst, dst_pitch and dst_item are multiples of 4: whole-dword stores
};

// two neighbouring source pixels, any alignment (gfx950 serves unaligned 2-byte global loads)
static __device__ inline uint32_t load_pair(const uint8_t *p) { uint16_t v; __builtin_memcpy(&v, p, 2); return v; }
// eight neighbouring source pixels of a row, any alignment
static __device__ inline uint64_t load_seg(const uint8_t *p) { uint64_t v; __builtin_memcpy(&v, p, 8); return v; }

__global__ __launch_bounds__(RM_TX * RM_TY) void k_remap(const RemapArgs A)
{
    const int x0 = ((int)blockIdx.x * RM_TX + (int)threadIdx.x) * 4, y = (int)blockIdx.y * RM_TY + (int)threadIdx.y;
    if (x0 >= A.w || y >= A.h) return;
    const int nv = A.w - x0 < 4 ? A.w - x0 : 4;                 // pixels this lane owns (the row tail: fewer than 4)
    const size_t m = (size_t)y * A.mpitch + x0;                 // mpitch is a multiple of 4: both vector loads are aligned
    const uint4 mxy = *(const uint4 *)(A.ixy + m);
    const uint2 mab = *(const uint2 *)(A.ab + m);
    uint32_t xy[4] = {mxy.x, mxy.y, mxy.z, mxy.w};
    uint32_t ab[4] = {mab.x & 0xffffu, mab.x >> 16, mab.y & 0xffffu, mab.y >> 16};
#pragma unroll
    for (int j = 1; j < 4; j++) if (j >= nv) { xy[j] = xy[0]; ab[j] = ab[0]; }   // a row-tail lane: its spare slots must not widen its footprint
    int o0[4], o1[4], w00[4], w01[4], w10[4], w11[4];           // per pixel: the pair's offset in rows iy / iy + 1, the four weights
    int cx_[4], ra[4], rb[4];                                    // the pair's column and its two rows, clamped into the image
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int ix = (int)(int16_t)(xy[j] & 0xffffu), iy = (int)(int16_t)(xy[j] >> 16);
        const int a = (int)(ab[j] & 31u), b = (int)(ab[j] >> 5);
        // The pair loaded is columns (cx, cx + 1).  Inside the row that is (tap ix, tap ix + 1); at ix == -1 its low byte is tap
        // ix + 1 (tap ix is outside); at ix == w - 1 its high byte is tap ix (tap ix + 1 is outside); further out no tap is inside.
        const int cx = min(max(ix, 0), A.w - 2);
        const int wlo = ix == cx ? 32 - a : ix == -1 ? a : 0;
        const int whi = ix == cx ? a : ix == A.w - 1 ? 32 - a : 0;
        const int wy0 = (unsigned)iy < (unsigned)A.h ? 32 - b : 0, wy1 = (unsigned)(iy + 1) < (unsigned)A.h ? b : 0;
        cx_[j] = cx; ra[j] = min(max(iy, 0), A.h - 1); rb[j] = min(max(iy + 1, 0), A.h - 1);
        o0[j] = ra[j] * A.src_pitch + cx;
        o1[j] = rb[j] * A.src_pitch + cx;
        w00[j] = wlo * wy0; w01[j] = whi * wy0; w10[j] = wlo * wy1; w11[j] = whi * wy1;
    }
    // Rectification maps are smooth: the 8 pairs of a lane usually lie within 8 columns of 3 consecutive source rows.  Such a lane
    // reads those three 8-byte row segments (3 loads instead of 8) and picks each pair out of them by a shift; any other lane --
    // strong magnification or rotation, a hand-made map, an image narrower than 8 -- gathers its pairs one by one.
    const int c0 = min(min(min(cx_[0], cx_[1]), min(cx_[2], cx_[3])), A.w - 8);          // [c0, c0 + 8) stays inside the row
    const int R0 = min(min(ra[0], ra[1]), min(ra[2], ra[3])), R1 = min(R0 + 1, A.h - 1), R2 = min(R0 + 2, A.h - 1);
    bool compact = A.w >= 8;
    int sh[4], sel0[4], sel1[4];                                  // per pixel: bit offset of its pair in a segment; which segment holds row ra / rb
#pragma unroll
    for (int j = 0; j < 4; j++) {
        compact = compact && cx_[j] - c0 <= 6 && ra[j] <= R1 && rb[j] <= R2;             // (ra >= R0, rb >= ra: rows R0..R2 cover them)
        sh[j] = 8 * (cx_[j] - c0);
        sel0[j] = ra[j] == R0 ? 0 : 1;
        sel1[j] = rb[j] == R0 ? 0 : rb[j] == R1 ? 1 : 2;
    }
    const int q0 = R0 * A.src_pitch + c0, q1 = R1 * A.src_pitch + c0, q2 = R2 * A.src_pitch + c0;
    const int i0 = (int)blockIdx.z * A.per_wg, i1 = min(A.n_items, i0 + A.per_wg);
    const long long dpx = (long long)y * A.dst_pitch + x0;
    for (int it = i0; it < i1; it++) {
        const uint8_t *s = A.src + (long long)it * A.src_item;
        uint32_t out = 0, r0[4], r1[4];
        if (compact) {
            const uint64_t s0 = load_seg(s + q0), s1 = load_seg(s + q1), s2 = load_seg(s + q2);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                r0[j] = (uint32_t)((sel0[j] == 0 ? s0 : s1) >> sh[j]) & 0xffffu;
                r1[j] = (uint32_t)((sel1[j] == 0 ? s0 : sel1[j] == 1 ? s1 : s2) >> sh[j]) & 0xffffu;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) { r0[j] = load_pair(s + o0[j]); r1[j] = load_pair(s + o1[j]); }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            // (p00*(32-a)*(32-b)*32 + ... + (1 << 14)) >> 15 with the common factor 32 divided out: the same integer
            const uint32_t v = (r0[j] & 0xffu) * w00[j] + (r0[j] >> 8) * w01[j] + (r1[j] & 0xffu) * w10[j] + (r1[j] >> 8) * w11[j];
            out |= ((v + 512u) >> 10) << (8 * j);
        }
        uint8_t *d = A.dst + (long long)it * A.dst_item + dpx;
        if (nv == 4 && A.dword_ok) *(uint32_t *)d = out;
        else for (int j = 0; j < nv; j++) d[j] = (uint8_t)(out >> (8 * j));
    }
}

int ov2_launch_remap(hipStream_t stream, const ov2_rectmap *m, const uint8_t *src_d, size_t src_pitch, size_t src_item, int n_items,
                     uint8_t *dst_d, size_t dst_pitch, size_t dst_item)
{
    OV2_REQUIRE(src_pitch * (size_t)m->h < ((size_t)1 << 31) && dst_pitch < ((size_t)1 << 31), OV2_EINVAL, "remap: an image of 2 GiB or more");
    RemapArgs A;
    A.ixy = m->ixy; A.ab = m->ab; A.w = m->w; A.h = m->h; A.mpitch = m->pitch;
    A.src = src_d; A.src_pitch = (int)src_pitch; A.src_item = (long long)src_item;
    A.dst = dst_d; A.dst_pitch = (int)dst_pitch; A.dst_item = (long long)dst_item;
    A.n_items = n_items;
    int groups = (n_items + RM_ITEMS - 1) / RM_ITEMS;
    if (groups > 65535) groups = 65535;
    A.per_wg = (n_items + groups - 1) / groups;
    groups = (n_items + A.per_wg - 1) / A.per_wg;
    A.dword_ok = (((uintptr_t)dst_d | dst_pitch | dst_item) & 3) == 0;
    const dim3 grid((m->w + 4 * RM_TX - 1) / (4 * RM_TX), (m->h + RM_TY - 1) / RM_TY, groups);
    hipLaunchKernelGGL(k_remap, grid, dim3(RM_TX, RM_TY), 0, stream, A);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}


extern "C" {

int ov2_rectmap_create(ov2_ctx *ctx, int w, int h, int form, const void *map1, const void *map2, ov2_rectmap **out)
{
    OV2_REQUIRE(out != nullptr, OV2_EINVAL, "out == NULL");
    *out = nullptr;
    OV2_REQUIRE(map1 && map2, OV2_EINVAL, "NULL map");
    OV2_REQUIRE(form == OV2_MAP_F32 || form == OV2_MAP_FIXED, OV2_EINVAL, "unknown map form");
    OV2_REQUIRE(w >= 2 && h >= 2 && w <= 32767 && h <= 32767, OV2_EINVAL, "map size outside [2, 32767]");
    // the whole contract is checked, and both forms are normalised, on the host before anything touches the device
    const int mp = (w + 3) & ~3;
    std::vector<uint32_t> ixy((size_t)mp * h, 0u);
    std::vector<uint16_t> ab((size_t)mp * h, (uint16_t)0);
    if (form == OV2_MAP_F32) {
        const float *mx = (const float *)map1, *my = (const float *)map2;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const float fx = mx[(size_t)y * w + x], fy = my[(size_t)y * w + x];
                OV2_REQUIRE(std::isfinite(fx) && std::isfinite(fy), OV2_EINVAL, "non-finite map value");
                OV2_REQUIRE(fabsf(fx) * 32.f < 2147483648.f && fabsf(fy) * 32.f < 2147483648.f, OV2_EINVAL, "map value * 32 does not fit an int");
                // cvRound(v * 32.f): the product is exact, the rounding to nearest with ties to even (the default rounding mode)
                const int sx = (int)lrintf(fx * 32.f), sy = (int)lrintf(fy * 32.f);
                int ix = sx >> 5, iy = sy >> 5;                              // arithmetic shifts: negative coordinates floor
                ix = ix < -32768 ? -32768 : ix > 32767 ? 32767 : ix;        // saturate_cast<short>
                iy = iy < -32768 ? -32768 : iy > 32767 ? 32767 : iy;
                ixy[(size_t)y * mp + x] = (uint32_t)(uint16_t)(int16_t)ix | ((uint32_t)(uint16_t)(int16_t)iy << 16);
                ab[(size_t)y * mp + x] = (uint16_t)((sy & 31) * 32 + (sx & 31));
            }
    } else {
        const int16_t *m1 = (const int16_t *)map1;
        const uint16_t *m2 = (const uint16_t *)map2;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const size_t i = (size_t)y * w + x;
                OV2_REQUIRE(m2[i] < 1024, OV2_EINVAL, "fixed-point map2 value >= 1024");
                ixy[(size_t)y * mp + x] = (uint32_t)(uint16_t)m1[2 * i] | ((uint32_t)(uint16_t)m1[2 * i + 1] << 16);
                ab[(size_t)y * mp + x] = m2[i];
            }
    }
    OV2_REQUIRE(ctx != nullptr, OV2_EINVAL, "ctx == NULL");
    OV2_HIP_CHECK(hipSetDevice(ctx->device));
    ov2_rectmap *m = new (std::nothrow) ov2_rectmap();
    OV2_REQUIRE(m != nullptr, OV2_ENOMEM, "out of host memory");
    m->device = ctx->device; m->w = w; m->h = h; m->pitch = mp;
    hipError_t e = hipMalloc((void **)&m->ixy, ixy.size() * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&m->ab, ab.size() * 2);
    if (e == hipSuccess) e = hipMemcpy(m->ixy, ixy.data(), ixy.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(m->ab, ab.data(), ab.size() * 2, hipMemcpyHostToDevice);
    if (e != hipSuccess) { ov2_set_error("ov2_rectmap_create: %s", hipGetErrorString(e)); ov2_rectmap_destroy(m); return OV2_ENOMEM; }
    *out = m;
    return OV2_OK;
}

void ov2_rectmap_destroy(ov2_rectmap *m)
{
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->ixy) (void)hipFree(m->ixy);
    if (m->ab) (void)hipFree(m->ab);
    delete m;
}

int ov2_rectify_d(ov2_ctx *ctx, const ov2_rectmap *map, const uint8_t *src_d, size_t src_pitch, size_t src_item_stride, int n_items,
                  uint8_t *dst_d, size_t dst_pitch, size_t dst_item_stride)
{
    OV2_REQUIRE(ctx && map && src_d && dst_d, OV2_EINVAL, "NULL argument");
    OV2_REQUIRE(src_d != dst_d, OV2_EINVAL, "src and dst must not overlap");
    OV2_REQUIRE(n_items >= 1, OV2_EINVAL, "n_items < 1");
    OV2_REQUIRE(src_pitch >= (size_t)map->w && dst_pitch >= (size_t)map->w, OV2_EINVAL, "stride < width");
    const size_t need_s = src_pitch * (size_t)(map->h - 1) + (size_t)map->w, need_d = dst_pitch * (size_t)(map->h - 1) + (size_t)map->w;
    OV2_REQUIRE(n_items == 1 || (src_item_stride >= need_s && dst_item_stride >= need_d), OV2_EINVAL, "item stride smaller than an image");
    OV2_REQUIRE(map->device == ctx->device, OV2_EINVAL, "the map lives on another device");
    OV2_HIP_CHECK(hipSetDevice(ctx->device));
    return ov2_launch_remap(ctx->stream, map, src_d, src_pitch, src_item_stride, n_items, dst_d, dst_pitch, dst_item_stride);
}

int ov2_rectify_h(ov2_ctx *ctx, const ov2_rectmap *map, const uint8_t *src_h, int src_stride, uint8_t *dst_h, int dst_stride)
{
    OV2_REQUIRE(ctx && map && src_h && dst_h, OV2_EINVAL, "NULL argument");
    OV2_REQUIRE(src_stride >= map->w && dst_stride >= map->w, OV2_EINVAL, "stride < width");
    OV2_REQUIRE(map->device == ctx->device, OV2_EINVAL, "the map lives on another device");
    OV2_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t w = (size_t)map->w, h = (size_t)map->h, spitch = up16(w);
    // download_image copies whole pitched rows when the two pitches agree: a device pitch that differs from dst_stride keeps
    // the caller's row padding as it was
    const size_t dpitch = spitch == (size_t)dst_stride ? spitch + 16 : spitch;
    const size_t simg = up256(spitch * h), dimg = up256(dpitch * h);
    int rc = ctx->reserve_device(simg + dimg);
    if (rc != OV2_OK) return rc;
    uint8_t *ds = (uint8_t *)ctx->d_scratch;
    rc = ctx->upload_image(ds, spitch, src_h, (size_t)src_stride, w, h);          // (src_h is free again: dst_h == src_h is fine)
    if (rc != OV2_OK) return rc;
    rc = ov2_launch_remap(ctx->stream, map, ds, spitch, 0, 1, ds + simg, dpitch, 0);
    if (rc != OV2_OK) return rc;
    return ctx->download_image(dst_h, (size_t)dst_stride, ds + simg, dpitch, w, h);   // (synchronises)
}

// the right image(s) of a stereo keyframe (src/ov2slam.cpp:255-256 + src/mapper.cpp:74-81): upload, remap, then what
// ov2_pyr_build_clahe_h / _hb (use_clahe) or ov2_pyr_build_h do with the rectified frames
int ov2_pyr_build_rect_h(ov2_ctx *ctx, ov2_pyr *p, const ov2_rectmap *map, int n_items, const uint8_t *const *img_h, int stride,
                         int use_clahe, double clip_limit, int tiles_x, int tiles_y)
{
    OV2_REQUIRE(ctx && p && map && img_h, OV2_EINVAL, "NULL argument");
    OV2_REQUIRE(p->parent == nullptr, OV2_EINVAL, "an item view is read-only");
    OV2_REQUIRE(map->w == p->w && map->h == p->h, OV2_EINVAL, "map and pyramid differ in size");
    OV2_REQUIRE(n_items >= 1 && n_items <= p->d.batch, OV2_EINVAL, "n_items out of range");
    OV2_REQUIRE(stride >= p->w && (!use_clahe || (tiles_x > 0 && tiles_y > 0 && tiles_x <= p->w && tiles_y <= p->h)), OV2_EINVAL, "bad geometry");
    for (int b = 0; b < n_items; b++) OV2_REQUIRE(img_h[b] != nullptr, OV2_EINVAL, "NULL image");
    OV2_REQUIRE(map->device == ctx->device, OV2_EINVAL, "the map lives on another device");
    OV2_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t pitch = up16((size_t)p->w), img = up256(pitch * p->h), n = (size_t)n_items;
    const size_t lut_bytes = use_clahe ? n * tiles_x * tiles_y * 256 : 0;
    int rc = ctx->reserve_device(2 * img * n + lut_bytes);
    if (rc != OV2_OK) return rc;
    uint8_t *raw = (uint8_t *)ctx->d_scratch, *ds = raw + img * n;
    rc = ctx->upload_images(raw, pitch, img, img_h, n_items, (size_t)stride, (size_t)p->w, (size_t)p->h);
    if (rc != OV2_OK) return rc;
    rc = ov2_launch_remap(ctx->stream, map, raw, pitch, img, n_items, ds, pitch, img);
    if (rc != OV2_OK) return rc;
    ov2_pyr q = *p;                                   // items [0, n_items): the launchers size their grids from d.batch
    q.d.batch = n_items;
    if (use_clahe) {
        const PyrLevelDesc &L0 = q.d.lv[0];
        int l1_done = 0;
        rc = ov2_launch_clahe(ctx, ds, p->w, p->h, (int)pitch, img, n_items, clip_limit, tiles_x, tiles_y, q.d.base + L0.img_roi, L0.img_pitch,
                              (size_t)q.d.item_stride, ds + img * n, q.d.win, &q.d, &l1_done);
        if (rc != OV2_OK) return rc;
        rc = ov2_launch_pyr_build(ctx, &q, nullptr, 0, 0, l1_done);
    } else
        rc = ov2_launch_pyr_build(ctx, &q, ds, (int)pitch, img);
    if (rc != OV2_OK) return rc;
    return ov2_pyr_mark_ready(ctx, p);
}

} // extern "C"
