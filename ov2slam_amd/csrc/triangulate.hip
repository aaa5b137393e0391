// triangulate.hip -- the mapper's triangulation of a new keyframe for gfx950 (the reference's src/mapper.cpp:191-461):
//   k_triangulate   Mapper::triangulateStereo (:346-461) then Mapper::triangulateTemporal (:191-344), ONE LANE PER KEYPOINT, fp64.
// Each iteration of the two reference loops reads and mutates only the map point of its own keypoint (updateMapPoint,
// removeStereoKeypointById, removeMapPointObs), so one lane per keypoint reproduces the sequential loops: a keypoint that the
// stereo pass rejects stays 2-D and goes on to the temporal pass in the same lane.  The map look-ups that decide who is a
// temporal candidate (:243-295) stay on the host; the lane receives the source keyframe and the source keypoint.
// MultiViewGeometry::triangulate is OpenGV's triangulate2 (the USE_OPENGV build, src/multi_view_geometry.cpp:53-100), the closed
// form midpoint.  Sophus / Eigen arithmetic is restated from the vendored headers (so3.hpp, se3.hpp); sums of three products
// run serially.  tests/tri_ref.py is the same arithmetic in numpy.
// Layout: per-point fields one array each (float2 pixels, 3-double bearings, contiguous records), so a wavefront's loads of
// one field cover consecutive bytes; grid.y = batch item.
#include "mvg_dev.hpp"

#pragma clang fp contract(off)

#define TRI_BLOCK 64

struct TriParams {
    int stereo, rect;
    float emax;
    double K[4], iK[9], Kr[4];
    TriSE3 Tlr, Trl, Tcic0;
};

// opengv::triangulation::triangulate2 with (R12, t12) = the Tlr handed to MultiViewGeometry::triangulate (:85-100)
__device__ __forceinline__ TriD3 tri_triangulate2(const double R12[9], TriD3 t12, TriD3 f1, TriD3 f2)
{
    const TriD3 f2u = tri_matvec(R12, f2);
    const double b0 = tri_dot(t12, f1), b1 = tri_dot(t12, f2u);
    const double a00 = tri_dot(f1, f1), a10 = tri_dot(f1, f2u);
    const double a01 = -a10, a11 = -tri_dot(f2u, f2u);
    const double invdet = 1. / (a00 * a11 - a10 * a01);            // Eigen compute_inverse<.., 2>
    const double i00 = a11 * invdet, i10 = -a10 * invdet, i01 = -a01 * invdet, i11 = a00 * invdet;
    const double l0 = i00 * b0 + i01 * b1, l1 = i10 * b0 + i11 * b1;
    return TriD3{(l0 * f1.x + (t12.x + l1 * f2u.x)) / 2., (l0 * f1.y + (t12.y + l1 * f2u.y)) / 2., (l0 * f1.z + (t12.z + l1 * f2u.z)) / 2.};
}
// items[b] = {first point slot, point count, first row of the source table, 0}; twc: 7 doubles per item; srcT: 14 doubles per source
// keyframe (Twc, Tcw).  Outputs: status / wpt / invdepth per point slot (zeros where no point was created).
__global__ __launch_bounds__(TRI_BLOCK) void k_triangulate(TriParams P, const int4 *__restrict__ items, const double *__restrict__ twc,
                                                           const double *__restrict__ srcT, const float2 *__restrict__ unpx,
                                                           const double *__restrict__ bv, const float2 *__restrict__ runpx,
                                                           const double *__restrict__ rbv, const float2 *__restrict__ src_unpx,
                                                           const double *__restrict__ src_bv, const int *__restrict__ src,
                                                           const uint8_t *__restrict__ is_stereo, uint8_t *__restrict__ status,
                                                           double *__restrict__ wpt, double *__restrict__ invdepth)
{
    const int4 it = items[blockIdx.y];
    const int il = blockIdx.x * TRI_BLOCK + threadIdx.x;
    if (il >= it.y) return;
    const int i = it.x + il;
    const float2 u = unpx[i];
    const TriD3 b{bv[3 * i], bv[3 * i + 1], bv[3 * i + 2]};
    const TriSE3 Twc = tri_load(twc + 7 * (size_t)blockIdx.y);
    int st = 0;
    TriD3 w{0., 0., 0.};
    double inv = 0.;
    if (is_stereo[i]) {                                             // Mapper::triangulateStereo, :405-456
        st = OV2_TRI_STEREO_TRIED;
        const float2 ru = runpx[i];
        bool ok = true;
        TriD3 left;
        if (P.rect) {
            const float disp = u.x - ru.x;                          // :411
            if (disp < 0.f) ok = false;
            const float z = (float)(P.K[0] * sqrt(tri_dot(P.Tcic0.t, P.Tcic0.t)) / (double)fabsf(disp));   // :417; disp == 0: NaN point, kept
            const double zd = (double)z, ux = (double)u.x, uy = (double)u.y;
            left = TriD3{(zd * P.iK[0] * ux + zd * P.iK[1] * uy) + zd * P.iK[2] * 1.,
                         (zd * P.iK[3] * ux + zd * P.iK[4] * uy) + zd * P.iK[5] * 1.,
                         (zd * P.iK[6] * ux + zd * P.iK[7] * uy) + zd * P.iK[8] * 1.};
        } else {
            double R[9];
            tri_rotmat(P.Tlr.q, R);
            left = tri_triangulate2(R, P.Tlr.t, b, TriD3{rbv[3 * i], rbv[3 * i + 1], rbv[3 * i + 2]});
        }
        if (ok) {
            const TriD3 right = tri_act(P.Trl, left);               // :426
            if (left.z < 0.1 || right.z < 0.1) ok = false;
        }
        if (ok) {
            const float ldist = (float)tri_pdist(tri_project(P.K, left), u);                       // :434-437
            const float rdist = (float)tri_pdist(tri_project(P.Kr, tri_act(P.Tcic0, left)), ru);
            if (ldist > P.emax || rdist > P.emax) ok = false;
        }
        if (ok) {
            st |= OV2_TRI_STEREO_OK;
            w = tri_act(Twc, left);                                 // :448-450
            inv = 1. / left.z;
        }
    }
    const int s = src[i];
    if (!(st & OV2_TRI_STEREO_OK) && s >= 0) {                      // Mapper::triangulateTemporal, :273-333
        const double *T = srcT + 14 * (size_t)(it.z + s);
        const TriSE3 Tcicj = tri_mul(tri_load(T + 7), Twc);         // :278
        if (P.stereo && sqrt(tri_dot(Tcicj.t, Tcicj.t)) < 0.01) {   // :287
            st |= OV2_TRI_NO_MOTION;
        } else {
            const TriQ qi = tri_qnormalize(-Tcicj.q.x, -Tcicj.q.y, -Tcicj.q.z, Tcicj.q.w);          // Tcjci = Tcicj.inverse(), :280
            const TriSE3 Tcjci{tri_qact(qi, TriD3{Tcicj.t.x * -1., Tcicj.t.y * -1., Tcicj.t.z * -1.}), qi};
            double R[9];
            tri_rotmat(Tcicj.q, R);                                 // :281
            const float2 ku = src_unpx[i];
            const TriD3 kb{src_bv[3 * i], src_bv[3 * i + 1], src_bv[3 * i + 2]};
            const double parallax = tri_pdist(ku, tri_project(P.K, tri_matvec(R, b)));             // :299-300
            st |= OV2_TRI_TEMPORAL_TRIED;
            const TriD3 left = tri_triangulate2(R, Tcicj.t, kb, b); // :305
            const TriD3 right = tri_act(Tcjci, left);
            bool ok = !(left.z < 0.1 || right.z < 0.1);
            if (ok) {
                const float ldist = (float)tri_pdist(tri_project(P.K, left), ku);                  // :320-323
                const float rdist = (float)tri_pdist(tri_project(P.K, right), u);
                ok = !(ldist > P.emax || rdist > P.emax);
            }
            if (ok) {
                st |= OV2_TRI_TEMPORAL_OK;
                w = tri_act(tri_load(T), left);                     // pkf->projCamToWorld, :334
                inv = 1. / left.z;
            } else if (parallax > 20.) {
                st |= OV2_TRI_REMOVE_OBS;                           // removeMapPointObs(lmid, frame.kfid_), :311-313 / :326-328
            }
        }
    }
    status[i] = (uint8_t)st;
    wpt[3 * i] = w.x; wpt[3 * i + 1] = w.y; wpt[3 * i + 2] = w.z;
    invdepth[i] = inv;
}

// the kernel's parameter block of a call's ov2_tri_params
static TriParams tri_make_params(const ov2_tri_params *params)
{
    TriParams P;
    P.stereo = params->stereo ? 1 : 0; P.rect = params->rect ? 1 : 0; P.emax = params->fmax_reproj_err;
    for (int j = 0; j < 4; j++) { P.K[j] = params->K[j]; P.Kr[j] = params->Kr[j]; }
    for (int j = 0; j < 9; j++) P.iK[j] = params->iK[j];
    P.Tlr = tri_load(params->Tlr); P.Tcic0 = tri_load(params->Tcic0);
    {   // Trl = Tlr.inverse() (:379), the same arithmetic as the device's Tcjci, on the host once per call
        const TriQ q = P.Tlr.q;
        const double nn = std::sqrt(((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w);
        const TriQ qi{-q.x / nn, -q.y / nn, -q.z / nn, q.w / nn};
        const TriD3 p{P.Tlr.t.x * -1., P.Tlr.t.y * -1., P.Tlr.t.z * -1.}, qv{qi.x, qi.y, qi.z};
        TriD3 uv{qv.y * p.z - qv.z * p.y, qv.z * p.x - qv.x * p.z, qv.x * p.y - qv.y * p.x};
        uv = TriD3{uv.x + uv.x, uv.y + uv.y, uv.z + uv.z};
        const TriD3 c{qv.y * uv.z - qv.z * uv.y, qv.z * uv.x - qv.x * uv.z, qv.x * uv.y - qv.y * uv.x};
        P.Trl = TriSE3{TriD3{(p.x + qi.w * uv.x) + c.x, (p.y + qi.w * uv.y) + c.y, (p.z + qi.w * uv.z) + c.z}, qi};
    }
    return P;
}

// launcher for trackb.hip (ov2_btracker_stereo_keyframe): k_triangulate on device arrays, items_d = {first slot, count, first source
// row, 0} per item; n_max: the largest count an item may carry
int ov2_launch_triangulate(hipStream_t s, const ov2_tri_params *params, const void *items_d, const double *twc_d, const double *srcT_d,
                           const float *unpx_d, const double *bv_d, const float *runpx_d, const double *rbv_d, const float *src_unpx_d,
                           const double *src_bv_d, const int *src_d, const uint8_t *is_stereo_d, uint8_t *status_d, double *wpt_d,
                           double *invdepth_d, int n_max, int n_items)
{
    const TriParams P = tri_make_params(params);
    hipLaunchKernelGGL(k_triangulate, dim3((n_max + TRI_BLOCK - 1) / TRI_BLOCK, n_items), dim3(TRI_BLOCK), 0, s, P, (const int4 *)items_d, twc_d,
                       srcT_d, (const float2 *)unpx_d, bv_d, (const float2 *)runpx_d, rbv_d, (const float2 *)src_unpx_d, src_bv_d, src_d,
                       is_stereo_d, status_d, wpt_d, invdepth_d);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

int ov2_triangulate_keyframe_batch(ov2_ctx *ctx, const ov2_tri_params *params, int n_items, const ov2_tri_keyframe *kfs,
                                   ov2_tri_result *results)
{
    OV2_REQUIRE(ctx && params, OV2_EINVAL, "NULL argument");
    OV2_REQUIRE(n_items >= 0, OV2_EINVAL, "n_items < 0");
    if (n_items == 0) return OV2_OK;
    OV2_REQUIRE(kfs && results, OV2_EINVAL, "NULL keyframe / result array");
    OV2_REQUIRE(n_items <= 65535, OV2_EUNSUPPORTED, "more than 65535 keyframes in one call");
    size_t N = 0, S = 0;
    int n_max = 0;
    for (int b = 0; b < n_items; b++) {
        const ov2_tri_keyframe &k = kfs[b];
        const ov2_tri_result &r = results[b];
        OV2_REQUIRE(k.n >= 0 && k.n_src >= 0, OV2_EINVAL, "n < 0 or n_src < 0");
        OV2_REQUIRE(k.Twc, OV2_EINVAL, "Twc == NULL");
        if (k.n > 0) {
            OV2_REQUIRE(k.unpx && k.bv, OV2_EINVAL, "NULL unpx / bv");
            OV2_REQUIRE(r.status && r.wpt && r.invdepth, OV2_EINVAL, "NULL result buffer");
        }
        OV2_REQUIRE(k.n_src == 0 || (k.src_Twc && k.src_Tcw), OV2_EINVAL, "NULL source keyframe table");
        for (int i = 0; i < k.n; i++) {
            if (k.is_stereo && k.is_stereo[i]) {
                OV2_REQUIRE(k.runpx && k.rbv, OV2_EINVAL, "a point flagged stereo without right data (runpx / rbv)");
                OV2_REQUIRE(params->stereo, OV2_EINVAL, "a point flagged stereo in mono mode");
            }
            if (k.src) {
                OV2_REQUIRE(k.src[i] >= -1 && k.src[i] < k.n_src, OV2_EINVAL, "source keyframe index outside the table");
                OV2_REQUIRE(k.src[i] < 0 || (k.src_unpx && k.src_bv), OV2_EINVAL, "a temporal point without source keypoint (src_unpx / src_bv)");
            }
        }
        OV2_REQUIRE(N + (size_t)k.n <= 0x7fffffff, OV2_EUNSUPPORTED, "more than 2^31 points in one call");
        N += (size_t)k.n; S += (size_t)k.n_src;
        n_max = k.n > n_max ? k.n : n_max;
    }
    const TriParams P = tri_make_params(params);
    // staging: [items 16B][Twc 56B][source table 112B] [unpx 8][bv 24][runpx 8][rbv 24][src_unpx 8][src_bv 24][src 4][stereo 1] per point,
    // then the outputs [status 1][wpt 24][invdepth 8] per point; every section 16-byte aligned
    const size_t B = (size_t)n_items;
    StageCursor c(16);
    const size_t o_it = c.take(16 * B), o_tw = c.take(56 * B), o_st = c.take(112 * S), o_u = c.take(8 * N), o_b = c.take(24 * N);
    const size_t o_ru = c.take(8 * N), o_rb = c.take(24 * N), o_su = c.take(8 * N), o_sb = c.take(24 * N), o_s = c.take(4 * N), o_fl = c.take(N);
    const size_t o_out = c.take(N), o_w = c.take(24 * N), o_inv = c.take(8 * N), total = c.off;
    Stage st;
    int rc = st.open(ctx, total, total);  if (rc) return rc;
    uint8_t *hs = st.h, *ds = st.d;
    size_t p0 = 0, s0 = 0;
    for (int b = 0; b < n_items; b++) {
        const ov2_tri_keyframe &k = kfs[b];
        const size_t n = (size_t)k.n, m = (size_t)k.n_src;
        const int4 it = make_int4((int)p0, k.n, (int)s0, 0);
        memcpy(hs + o_it + 16 * b, &it, 16);
        memcpy(hs + o_tw + 56 * b, k.Twc, 56);
        for (size_t j = 0; j < m; j++) {
            memcpy(hs + o_st + 112 * (s0 + j), k.src_Twc + 7 * j, 56);
            memcpy(hs + o_st + 112 * (s0 + j) + 56, k.src_Tcw + 7 * j, 56);
        }
        if (n) {
            memcpy(hs + o_u + 8 * p0, k.unpx, 8 * n);
            memcpy(hs + o_b + 24 * p0, k.bv, 24 * n);
            if (k.runpx) memcpy(hs + o_ru + 8 * p0, k.runpx, 8 * n); else memset(hs + o_ru + 8 * p0, 0, 8 * n);
            if (k.rbv) memcpy(hs + o_rb + 24 * p0, k.rbv, 24 * n); else memset(hs + o_rb + 24 * p0, 0, 24 * n);
            if (k.src_unpx) memcpy(hs + o_su + 8 * p0, k.src_unpx, 8 * n); else memset(hs + o_su + 8 * p0, 0, 8 * n);
            if (k.src_bv) memcpy(hs + o_sb + 24 * p0, k.src_bv, 24 * n); else memset(hs + o_sb + 24 * p0, 0, 24 * n);
            if (k.src) memcpy(hs + o_s + 4 * p0, k.src, 4 * n); else memset(hs + o_s + 4 * p0, 0xff, 4 * n);    // -1: no source
            if (k.is_stereo) memcpy(hs + o_fl + p0, k.is_stereo, n); else memset(hs + o_fl + p0, 0, n);
        }
        p0 += n; s0 += m;
    }
    rc = st.upload(0, o_out);  if (rc) return rc;
    if (n_max > 0) {
        hipLaunchKernelGGL(k_triangulate, dim3((n_max + TRI_BLOCK - 1) / TRI_BLOCK, n_items), dim3(TRI_BLOCK), 0, ctx->stream, P,
                           (const int4 *)(ds + o_it), (const double *)(ds + o_tw), (const double *)(ds + o_st), (const float2 *)(ds + o_u),
                           (const double *)(ds + o_b), (const float2 *)(ds + o_ru), (const double *)(ds + o_rb), (const float2 *)(ds + o_su),
                           (const double *)(ds + o_sb), (const int *)(ds + o_s), (const uint8_t *)(ds + o_fl), ds + o_out,
                           (double *)(ds + o_w), (double *)(ds + o_inv));
        OV2_HIP_CHECK(hipGetLastError());
        rc = st.download(o_out, total, o_out);  if (rc) return rc;
    }
    rc = st.sync();  if (rc) return rc;
    p0 = 0;
    for (int b = 0; b < n_items; b++) {
        const size_t n = (size_t)kfs[b].n;
        ov2_tri_result &r = results[b];
        r.n_stereo = r.n_stereo_good = r.n_candidates = r.n_temporal_good = 0;
        if (!n) continue;
        memcpy(r.status, hs + o_out + p0, n);
        memcpy(r.wpt, hs + o_w + 24 * p0, 24 * n);
        memcpy(r.invdepth, hs + o_inv + 8 * p0, 8 * n);
        for (size_t i = 0; i < n; i++) {
            const uint8_t s = r.status[i];
            r.n_stereo += (s & OV2_TRI_STEREO_TRIED) ? 1 : 0;
            r.n_stereo_good += (s & OV2_TRI_STEREO_OK) ? 1 : 0;
            r.n_candidates += (s & OV2_TRI_TEMPORAL_TRIED) ? 1 : 0;
            r.n_temporal_good += (s & OV2_TRI_TEMPORAL_OK) ? 1 : 0;
        }
        p0 += n;
    }
    return OV2_OK;
}

int ov2_triangulate_keyframe(ov2_ctx *ctx, const ov2_tri_params *params, const ov2_tri_keyframe *kf, ov2_tri_result *result)
{
    OV2_REQUIRE(kf && result, OV2_EINVAL, "NULL keyframe / result");
    return ov2_triangulate_keyframe_batch(ctx, params, 1, kf, result);
}
