// priors.hip -- the priors that the reference's KLT calls start from, for gfx950:
//   k_prior_frame    VisualFrontEnd::kltTracking (src/visual_front_end.cpp:156-184): Frame::projWorldToImageDist of the map point of
//                    every 3-D keypoint with the predicted pose, Frame::isInImage.  No depth gate, as in the reference.
//   k_prior_stereo   MapManager::stereoMatching (src/map_manager.cpp:396-489): projWorldToRightImageDist / isInRightImage, and without
//                    rectification the inverse-distance-weighted depth of the 3-D neighbours in the 2 x 2 cell block of
//                    Frame::getSurroundingKeypoints(const Keypoint&) (frame.cpp:594-622) through projCamToRightImageDist.
// ONE LANE PER KEYPOINT, grid.y = item.  The neighbour walk is serial per lane: at most four short cell lists, and its order fixes
// the bits of the two double sums.  No atomics, no LDS.  include/ov2slam_hip.h states the arithmetic; tests/priors_ref.py is the
// same in numpy.  k_prior_frame also runs inside the lock-step step (trackb.hip: ov2_btracker_track_frame_map).
#include "keypoint_dev.hpp"
#include "mvg_dev.hpp"
#include <math.h>

#pragma clang fp contract(off)

#define PRI_THREADS 256

struct PriPose { double v[7]; };
// 16 bytes: first keypoint and count; first entry of the item's cell_start and of its cell_kp (stereo form)
struct PriItemD { int p0, n, cell0, ck0; };

// Frame::isInImage / isInRightImage (frame.cpp:840-848): the float pixel against the double image size; false for NaN
__device__ __forceinline__ bool pri_in_image(float2 p, double img_w, double img_h)
{
    return p.x >= 0.f && p.y >= 0.f && (double)p.x < img_w && (double)p.y < img_h;
}

__global__ __launch_bounds__(PRI_THREADS) void k_prior_frame(KpCalib c, double img_w, double img_h, int use_prior,
                                                             const PriItemD *__restrict__ items, const double *__restrict__ Tcw,
                                                             const float2 *__restrict__ px, const uint8_t *__restrict__ is3d,
                                                             const double *__restrict__ wpt, float2 *__restrict__ prior,
                                                             uint8_t *__restrict__ has_prior)
{
    const PriItemD it = items[blockIdx.y];
    const int il = blockIdx.x * PRI_THREADS + threadIdx.x;
    if (il >= it.n) return;
    const size_t g = (size_t)it.p0 + (size_t)il;
    float2 out = px[g];
    uint8_t hp = 0;
    if (use_prior && is3d[g]) {                                                    // :161-163
        const TriSE3 T = tri_load(Tcw + 7 * (size_t)blockIdx.y);
        const TriD3 cam = tri_act(T, TriD3{wpt[3 * g], wpt[3 * g + 1], wpt[3 * g + 2]});
        const float2 pr = kp_project_dist(c, cam.x, cam.y, cam.z);                 // :165
        if (pri_in_image(pr, img_w, img_h)) { out = pr; hp = 1; }                  // :168
    }
    // (kltkf.hip's k_kf_join and the from-keyframe tracking kernels rely on exactly this for a slot without a projection, klt_use_prior
    // == 0 included: prior = the frame's own px and flag 0 -- kltTrackingFromKF starts such a slot there, visual_front_end.cpp:343-345)
    prior[g] = out;
    has_prior[g] = hp;
}

__global__ __launch_bounds__(PRI_THREADS) void k_prior_stereo(KpCalib c, PriPose Tcic0, double img_w, double img_h, float cellsize,
                                                              int nbw, int nbh, int rect, const PriItemD *__restrict__ items,
                                                              const double *__restrict__ Tcw, const float2 *__restrict__ px,
                                                              const float2 *__restrict__ unpx, const double *__restrict__ bv,
                                                              const double *__restrict__ wpt, const uint8_t *__restrict__ state,
                                                              const int *__restrict__ cell_start, const int *__restrict__ cell_kp,
                                                              float2 *__restrict__ prior, uint8_t *__restrict__ has_prior,
                                                              uint8_t *__restrict__ skip)
{
    const PriItemD it = items[blockIdx.y];
    const int il = blockIdx.x * PRI_THREADS + threadIdx.x;
    if (il >= it.n) return;
    const size_t p0 = (size_t)it.p0, g = p0 + (size_t)il;
    const float2 p = px[g];
    const int st = state[g];
    float2 out = p;
    uint8_t hp = 0;
    const TriSE3 T = tri_load(Tcw + 7 * (size_t)blockIdx.y), Tr = tri_load(Tcic0.v);
    if (st == 1) {                                                                 // :405-414
        const TriD3 cam = tri_act(T, TriD3{wpt[3 * g], wpt[3 * g + 1], wpt[3 * g + 2]});
        const TriD3 r = tri_act(Tr, cam);
        const float2 pr = kp_project_dist(c, r.x, r.y, r.z);
        if (pri_in_image(pr, img_w, img_h)) { out = pr; hp = 1; }
    }
    if (st != 2 && hp == 0 && !rect) {                                             // :438-484
        const float rf = floorf(p.y / cellsize), cf = floorf(p.x / cellsize);      // frame.cpp:599-600
        double weights = 0., mean_z = 0.;
        int nb = 0;
        if (fabsf(rf) <= 1048576.f && fabsf(cf) <= 1048576.f) {                    // false for NaN too
            const int rkp = (int)rf, ckp = (int)cf;
            const float2 u = unpx[g];
            const int *cs = cell_start + it.cell0, *ck = cell_kp + it.ck0;
            for (int r = rkp - 1; r <= rkp; r++)
                for (int cc = ckp - 1; cc <= ckp; cc++) {
                    if (r < 0 || cc < 0 || r >= nbh || cc >= nbw) continue;
                    const int idx = r * nbw + cc;
                    const int e = cs[idx + 1];
                    for (int j = cs[idx]; j < e; j++) {
                        const int k = ck[j];
                        if (k == il || state[p0 + (size_t)k] != 1) continue;       // frame.cpp:612, map_manager.cpp:447, :460
                        const size_t gk = p0 + (size_t)k;
                        const double coef = 1. / tri_pdist(unpx[gk], u);           // :462
                        weights += coef;
                        mean_z += coef * tri_act(T, TriD3{wpt[3 * gk], wpt[3 * gk + 1], wpt[3 * gk + 2]}).z;
                        nb++;
                    }
                }
        }
        if (nb > 0) {
            mean_z /= weights;                                                     // :469
            const double bz = bv[3 * g + 2];
            const TriD3 pred{mean_z * (bv[3 * g] / bz), mean_z * (bv[3 * g + 1] / bz), mean_z * (bz / bz)};   // :470
            const TriD3 r = tri_act(Tr, pred);
            const float2 pr = kp_project_dist(c, r.x, r.y, r.z);                   // :472
            if (pri_in_image(pr, img_w, img_h)) { out = pr; hp = 2; }
        }
    }
    prior[g] = out;
    has_prior[g] = hp;
    skip[g] = st == 2 ? 1 : 0;
}

// launcher for trackb.hip: the frame form on device arrays with n_max point slots per item (items_d: {b * n_max, n_h[b], 0, 0})
int ov2_launch_prior_frame(hipStream_t s, const KpCalib &c, double img_w, double img_h, int use_prior, const void *items_d,
                           const double *Tcw_d, const float *px_d, const uint8_t *is3d_d, const double *wpt_d, float *prior_d,
                           uint8_t *has_prior_d, int n_max, int n_items)
{
    hipLaunchKernelGGL(k_prior_frame, dim3((n_max + PRI_THREADS - 1) / PRI_THREADS, n_items), dim3(PRI_THREADS), 0, s, c, img_w, img_h,
                       use_prior ? 1 : 0, (const PriItemD *)items_d, Tcw_d, (const float2 *)px_d, is3d_d, wpt_d, (float2 *)prior_d, has_prior_d);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

// launcher for trackb.hip (ov2_btracker_stereo_keyframe): the stereo form on device arrays with n_max point slots per item
// (items_d: PriItemD per item, written on the device; Tcic0: 7 doubles; cell_start_d / cell_kp_d unread with rect)
int ov2_launch_prior_stereo(hipStream_t s, const KpCalib &c, const double *Tcic0, double img_w, double img_h, int ncellsize, int nbw, int nbh,
                            int rect, const void *items_d, const double *Tcw_d, const float *px_d, const float *unpx_d, const double *bv_d,
                            const double *wpt_d, const uint8_t *state_d, const int *cell_start_d, const int *cell_kp_d, float *prior_d,
                            uint8_t *has_prior_d, uint8_t *skip_d, int n_max, int n_items)
{
    PriPose Tr;
    memcpy(Tr.v, Tcic0, 56);
    hipLaunchKernelGGL(k_prior_stereo, dim3((n_max + PRI_THREADS - 1) / PRI_THREADS, n_items), dim3(PRI_THREADS), 0, s, c, Tr, img_w, img_h,
                       (float)ncellsize, nbw, nbh, rect ? 1 : 0, (const PriItemD *)items_d, Tcw_d, (const float2 *)px_d, (const float2 *)unpx_d,
                       bv_d, wpt_d, state_d, cell_start_d, cell_kp_d, (float2 *)prior_d, has_prior_d, skip_d);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

// the camera of either params struct: the model, a coefficient count it takes, a positive image size
template <class Params>
static int pri_check_camera(const Params *params)
{
    OV2_REQUIRE(params, OV2_EINVAL, "NULL params");
    OV2_REQUIRE(params->model == OV2_CAM_PINHOLE || params->model == OV2_CAM_FISHEYE, OV2_EINVAL, "unknown camera model");
    OV2_REQUIRE(params->nD >= 0 && (params->nD == 0 || params->D), OV2_EINVAL, "bad distortion vector: nD < 0 or D == NULL");
    const int nD = params->nD;
    const bool ok = nD == 0 || (params->model == OV2_CAM_FISHEYE ? nD == 4 : (nD == 4 || nD == 5 || nD == 8 || nD == 12));
    OV2_REQUIRE(ok, OV2_EUNSUPPORTED, "unsupported coefficient count: pinhole takes 0 / 4 / 5 / 8 / 12 distortion coefficients, fisheye 0 / 4");
    OV2_REQUIRE(params->img_w > 0 && params->img_h > 0, OV2_EINVAL, "img_w / img_h not positive");     // false for NaN too
    return OV2_OK;
}

template <class Params>
static int pri_calib(const Params *params, KpCalib &c)
{
    const double iK[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};                  // the inverse model's matrix: not read here
    return ov2_kp_calib(params->model, params->K, params->D, params->nD, iK, c);
}

static int pri_frame_run(ov2_ctx *ctx, const ov2_klt_priors_params *params, int n_items, const ov2_klt_priors_item *items,
                         ov2_klt_priors_result *results)
{
    // the inputs first, the context last: a malformed input is reported without a device
    int rc = pri_check_camera(params);
    if (rc) return rc;
    OV2_REQUIRE(n_items >= 0, OV2_EINVAL, "n_items < 0");
    OV2_REQUIRE(n_items == 0 || (items && results), OV2_EINVAL, "NULL item / result array");
    OV2_REQUIRE(n_items <= 65535, OV2_EUNSUPPORTED, "more than 65535 items in one call");
    size_t N = 0;
    int n_max = 0;
    for (int b = 0; b < n_items; b++) {                                // the counts alone first: no array is read beyond the limit
        OV2_REQUIRE(items[b].n >= 0, OV2_EINVAL, "negative count (n)");
        N += (size_t)items[b].n;
        n_max = items[b].n > n_max ? items[b].n : n_max;
    }
    OV2_REQUIRE(N <= 0x7fffffff, OV2_EUNSUPPORTED, "more than 2^31 - 1 elements of one kind in one call");
    for (int b = 0; b < n_items; b++) {
        const ov2_klt_priors_item &k = items[b];
        OV2_REQUIRE(k.Tcw, OV2_EINVAL, "Tcw == NULL");
        if (k.n > 0) {
            OV2_REQUIRE(k.px && k.is3d && k.wpt, OV2_EINVAL, "NULL px / is3d / wpt");
            OV2_REQUIRE(results[b].prior && results[b].has_prior, OV2_EINVAL, "NULL result buffer (prior / has_prior)");
        }
    }
    OV2_REQUIRE(ctx, OV2_EINVAL, "NULL context");
    if (n_items == 0) return OV2_OK;
    KpCalib c;
    rc = pri_calib(params, c);
    if (rc) return rc;
    // staging: [items 16 B][Tcw 56 B] per item, [px 8][wpt 24][is3d 1] per keypoint, then the outputs [prior 8][has_prior 1]
    const size_t B = (size_t)n_items;
    StageCursor sc(16);
    const size_t o_it = sc.take(sizeof(PriItemD) * B), o_T = sc.take(56 * B), o_px = sc.take(8 * N), o_w = sc.take(24 * N), o_3d = sc.take(N);
    const size_t o_out = sc.take(8 * N), o_hp = sc.take(N), total = sc.off;
    Stage st;
    rc = st.open(ctx, total, total);  if (rc) return rc;
    uint8_t *hs = st.h, *ds = st.d;
    size_t p0 = 0;
    for (int b = 0; b < n_items; b++) {
        const ov2_klt_priors_item &k = items[b];
        const size_t n = (size_t)k.n;
        const PriItemD it = {(int)p0, k.n, 0, 0};
        memcpy(hs + o_it + sizeof(PriItemD) * b, &it, sizeof it);
        memcpy(hs + o_T + 56 * (size_t)b, k.Tcw, 56);
        if (n) {
            memcpy(hs + o_px + 8 * p0, k.px, 8 * n);
            memcpy(hs + o_w + 24 * p0, k.wpt, 24 * n);
            memcpy(hs + o_3d + p0, k.is3d, n);
        }
        p0 += n;
    }
    if (n_max > 0) {
        rc = st.upload(0, o_out);  if (rc) return rc;
        rc = ov2_launch_prior_frame(ctx->stream, c, params->img_w, params->img_h, params->klt_use_prior, ds + o_it, (const double *)(ds + o_T),
                                    (const float *)(ds + o_px), ds + o_3d, (const double *)(ds + o_w), (float *)(ds + o_out), ds + o_hp,
                                    n_max, n_items);
        if (rc) return rc;
        rc = st.download(o_out, total, o_out);  if (rc) return rc;
    }
    rc = st.sync();  if (rc) return rc;
    p0 = 0;
    for (int b = 0; b < n_items; b++) {
        const size_t n = (size_t)items[b].n;
        ov2_klt_priors_result &r = results[b];
        int np = 0;
        if (n) {
            memcpy(r.prior, hs + o_out + 8 * p0, 8 * n);
            memcpy(r.has_prior, hs + o_hp + p0, n);
            for (size_t i = 0; i < n; i++) np += r.has_prior[i] ? 1 : 0;
        }
        r.n_prior = np;
        p0 += n;
    }
    return OV2_OK;
}

// offsets[0 .. n]: starts at 0, never decreases
static bool pri_offsets_ok(const int *o, size_t n)
{
    if (o[0] != 0) return false;
    for (size_t i = 0; i < n; i++)
        if (o[i + 1] < o[i]) return false;
    return true;
}

static int pri_stereo_run(ov2_ctx *ctx, const ov2_stereo_priors_params *params, int n_items, const ov2_stereo_priors_item *items,
                          ov2_stereo_priors_result *results)
{
    int rc = pri_check_camera(params);
    if (rc) return rc;
    OV2_REQUIRE(params->ncellsize > 0, OV2_EINVAL, "ncellsize not positive");
    OV2_REQUIRE(params->img_w <= 65536 && params->img_h <= 65536, OV2_EINVAL, "img_w / img_h above 65536");
    OV2_REQUIRE(n_items >= 0, OV2_EINVAL, "n_items < 0");
    OV2_REQUIRE(n_items == 0 || (items && results), OV2_EINVAL, "NULL item / result array");
    OV2_REQUIRE(n_items <= 65535, OV2_EUNSUPPORTED, "more than 65535 items in one call");
    // Frame's grid (frame.cpp:41-43)
    const int nbw = (int)ceilf((float)params->img_w / (float)params->ncellsize);
    const int nbh = (int)ceilf((float)params->img_h / (float)params->ncellsize);
    const size_t ncells = (size_t)nbw * (size_t)nbh, B = (size_t)n_items, lim = 0x7fffffff;
    const bool rect = params->rect != 0;
    size_t N = 0;
    int n_max = 0;
    for (int b = 0; b < n_items; b++) {                                // the counts alone first: no array is read beyond the limit
        OV2_REQUIRE(items[b].n >= 0, OV2_EINVAL, "negative count (n)");
        N += (size_t)items[b].n;
        n_max = items[b].n > n_max ? items[b].n : n_max;
    }
    OV2_REQUIRE(N <= lim && B * (ncells + 1) <= lim, OV2_EUNSUPPORTED, "more than 2^31 - 1 elements of one kind in one call");
    size_t NCK = 0;
    for (int b = 0; b < n_items; b++) {
        const ov2_stereo_priors_item &k = items[b];
        OV2_REQUIRE(k.Tcw, OV2_EINVAL, "Tcw == NULL");
        if (k.n > 0) {
            OV2_REQUIRE(k.px && k.unpx && k.bv && k.wpt && k.state, OV2_EINVAL, "NULL px / unpx / bv / wpt / state");
            OV2_REQUIRE(rect || k.cell_start, OV2_EINVAL, "cell_start == NULL");
            OV2_REQUIRE(results[b].prior && results[b].has_prior && results[b].skip, OV2_EINVAL, "NULL result buffer (prior / has_prior / skip)");
            for (int i = 0; i < k.n; i++) OV2_REQUIRE(k.state[i] <= 2, OV2_EINVAL, "state > 2");
        }
        if (k.cell_start) {
            OV2_REQUIRE(pri_offsets_ok(k.cell_start, ncells), OV2_EINVAL, "cell_start does not start at 0 or decreases");
            const int n_ck = k.cell_start[ncells];
            OV2_REQUIRE(n_ck == 0 || k.cell_kp, OV2_EINVAL, "cell_kp == NULL");
            for (int i = 0; i < n_ck; i++)
                OV2_REQUIRE(k.cell_kp[i] >= 0 && k.cell_kp[i] < k.n, OV2_EINVAL, "cell_kp: keypoint row outside the keypoint table");
            NCK += (size_t)n_ck;
        }
    }
    OV2_REQUIRE(NCK <= lim, OV2_EUNSUPPORTED, "more than 2^31 - 1 elements of one kind in one call");
    OV2_REQUIRE(ctx, OV2_EINVAL, "NULL context");
    if (n_items == 0) return OV2_OK;
    KpCalib c;
    rc = pri_calib(params, c);
    if (rc) return rc;
    PriPose Tr;
    memcpy(Tr.v, params->Tcic0, 56);
    // staging: [items 16 B][Tcw 56 B] per item, [px 8][unpx 8][bv 24][wpt 24][state 1] per keypoint, [cell_start 4] per cell + 1,
    // [cell_kp 4], then the outputs [prior 8][has_prior 1][skip 1]
    const size_t CS = B * (ncells + 1);
    StageCursor sc(16);
    const size_t o_it = sc.take(sizeof(PriItemD) * B), o_T = sc.take(56 * B), o_px = sc.take(8 * N), o_un = sc.take(8 * N), o_bv = sc.take(24 * N);
    const size_t o_w = sc.take(24 * N), o_st = sc.take(N), o_cs = sc.take(4 * CS), o_ck = sc.take(4 * NCK);
    const size_t o_out = sc.take(8 * N), o_hp = sc.take(N), o_sk = sc.take(N), total = sc.off;
    Stage st;
    rc = st.open(ctx, total, total);  if (rc) return rc;
    uint8_t *hs = st.h, *ds = st.d;
    size_t p0 = 0, ck0 = 0;
    for (int b = 0; b < n_items; b++) {
        const ov2_stereo_priors_item &k = items[b];
        const size_t n = (size_t)k.n, n_ck = k.cell_start ? (size_t)k.cell_start[ncells] : 0;
        const PriItemD it = {(int)p0, k.n, (int)((size_t)b * (ncells + 1)), (int)ck0};
        memcpy(hs + o_it + sizeof(PriItemD) * b, &it, sizeof it);
        memcpy(hs + o_T + 56 * (size_t)b, k.Tcw, 56);
        if (n) {
            memcpy(hs + o_px + 8 * p0, k.px, 8 * n);
            memcpy(hs + o_un + 8 * p0, k.unpx, 8 * n);
            memcpy(hs + o_bv + 24 * p0, k.bv, 24 * n);
            memcpy(hs + o_w + 24 * p0, k.wpt, 24 * n);
            memcpy(hs + o_st + p0, k.state, n);
        }
        if (k.cell_start) memcpy(hs + o_cs + 4 * (size_t)it.cell0, k.cell_start, 4 * (ncells + 1));
        else memset(hs + o_cs + 4 * (size_t)it.cell0, 0, 4 * (ncells + 1));
        if (n_ck) memcpy(hs + o_ck + 4 * ck0, k.cell_kp, 4 * n_ck);
        p0 += n; ck0 += n_ck;
    }
    if (n_max > 0) {
        rc = st.upload(0, o_out);  if (rc) return rc;
        hipLaunchKernelGGL(k_prior_stereo, dim3((n_max + PRI_THREADS - 1) / PRI_THREADS, n_items), dim3(PRI_THREADS), 0, ctx->stream, c, Tr,
                           params->img_w, params->img_h, (float)params->ncellsize, nbw, nbh, rect ? 1 : 0, (const PriItemD *)(ds + o_it),
                           (const double *)(ds + o_T), (const float2 *)(ds + o_px), (const float2 *)(ds + o_un), (const double *)(ds + o_bv),
                           (const double *)(ds + o_w), (const uint8_t *)(ds + o_st), (const int *)(ds + o_cs), (const int *)(ds + o_ck),
                           (float2 *)(ds + o_out), ds + o_hp, ds + o_sk);
        OV2_HIP_CHECK(hipGetLastError());
        rc = st.download(o_out, total, o_out);  if (rc) return rc;
    }
    rc = st.sync();  if (rc) return rc;
    p0 = 0;
    for (int b = 0; b < n_items; b++) {
        const size_t n = (size_t)items[b].n;
        ov2_stereo_priors_result &r = results[b];
        int n1 = 0, n2 = 0, ns = 0;
        if (n) {
            memcpy(r.prior, hs + o_out + 8 * p0, 8 * n);
            memcpy(r.has_prior, hs + o_hp + p0, n);
            memcpy(r.skip, hs + o_sk + p0, n);
            for (size_t i = 0; i < n; i++) { n1 += r.has_prior[i] == 1; n2 += r.has_prior[i] == 2; ns += r.skip[i] ? 1 : 0; }
        }
        r.n_prior3d = n1; r.n_prior_nb = n2; r.n_skip = ns;
        p0 += n;
    }
    return OV2_OK;
}

extern "C" {

int ov2_klt_priors_batch(ov2_ctx *ctx, const ov2_klt_priors_params *params, int n_items, const ov2_klt_priors_item *items,
                         ov2_klt_priors_result *results)
{
    return pri_frame_run(ctx, params, n_items, items, results);
}

int ov2_klt_priors(ov2_ctx *ctx, const ov2_klt_priors_params *params, const ov2_klt_priors_item *item, ov2_klt_priors_result *result)
{
    OV2_REQUIRE(item && result, OV2_EINVAL, "NULL item / result");
    return pri_frame_run(ctx, params, 1, item, result);
}

int ov2_stereo_priors_batch(ov2_ctx *ctx, const ov2_stereo_priors_params *params, int n_items, const ov2_stereo_priors_item *items,
                            ov2_stereo_priors_result *results)
{
    return pri_stereo_run(ctx, params, n_items, items, results);
}

int ov2_stereo_priors(ov2_ctx *ctx, const ov2_stereo_priors_params *params, const ov2_stereo_priors_item *item,
                      ov2_stereo_priors_result *result)
{
    OV2_REQUIRE(item && result, OV2_EINVAL, "NULL item / result");
    return pri_stereo_run(ctx, params, 1, item, result);
}

} // extern "C"
