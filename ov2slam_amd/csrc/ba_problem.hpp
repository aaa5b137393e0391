// ba_problem.hpp -- the device-resident BA problem (ov2_ba_dev): validation, the landmark sort, the pool layout and the upload
// (ba_create, xyzba_create), the slices of a lock-step batch and the context's host thread pool.  A part of ba.hip (same
// translation unit): included there after BADev; sizes and path decisions come from ba_geom.hpp.
#pragma once
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

struct ov2_ba_dev {
    BADev D;
    void *pool = nullptr; size_t pool_bytes = 0;
    bool pool_owned = true;             // false: the pool lives in the context's grow-only device scratch (transient small problems)
    int n_res = 0;
    int *lm_order = nullptr;            // landmarks sorted by anchor keyframe (device)
    std::vector<double> h_poses0, h_lam0;
    int device = 0;
};

static void ba_destroy(ov2_ba_dev *dev);

// debug laps of a host entry point (ov2_ctx::debug): "[ov2 <who>] <what>  <ms> ms since entry" on stderr
struct BALap {
    const char *who; bool on;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void operator()(const char *what) const
    {
        if (on) fprintf(stderr, "[ov2 %s] %-34s %8.3f ms since entry\n", who, what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
};

// H2D copy of one array of a problem under construction on stream s; a failure destroys the half-built problem
static int ba_upload(ov2_ba_dev *dev, hipStream_t s, const void *dst, const void *src, size_t bytes)
{
    if (bytes == 0) return OV2_OK;
    const hipError_t e = hipMemcpyAsync((void *)dst, src, bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) return OV2_OK;
    ba_destroy(dev);
    ov2_set_error("H2D: %s", hipGetErrorString(e));
    return OV2_EHIP;
}
#define BA_UP(dst, src, bytes) do { const int rc_ = ba_upload(dev, s, (dst), (src), (bytes)); if (rc_ != OV2_OK) return rc_; } while (0)

// T_rl (t | quaternion) -> R | t of the device view; a zero quaternion stands for the identity
static void ba_set_extrinsic(BADev &D, const double *T_rl)
{
    const double *q = T_rl + 3, ident[4] = {0, 0, 0, 1};
    d_quat_to_R(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] > 0 ? q : ident, D.Rrl);
    D.trl[0] = T_rl[0]; D.trl[1] = T_rl[1]; D.trl[2] = T_rl[2];
}

// lock-step batch (ov2_local_ba_batch): the problems' pools and staging mirrors are consecutive slices of ONE device / pinned block
struct BASlice { uint8_t *dev_base; size_t dev_cap, dev_used; uint8_t *host_base; size_t host_cap, host_used; std::mutex m; };      // (the problems of a batch are prepared on several host threads)
#define BA_SLICE_FULL (-12345)          // (internal: the caller grows the blocks and starts over)

// persistent host threads of a context (ov2_ctx::ba_host_pool): the problems of a batch are prepared on them (spawning sixteen threads per
// batch was 0.3 ms of its first millisecond), and so are the slices of one large problem's sort (ba_create)
struct BAHostPool {
    std::vector<std::thread> th; std::mutex m; std::condition_variable cv_go, cv_done;
    const std::function<void(int)> *fn = nullptr; int n = 0, gen = 0, busy = 0; std::atomic<int> next{0}; bool quit = false;
    explicit BAHostPool(int nt)
    {
        try { spawn(nt); }
        catch (...) { { std::lock_guard<std::mutex> l(m); quit = true; } cv_go.notify_all(); for (auto &t : th) t.join(); th.clear(); throw; }
    }
    void spawn(int nt)
    {
        for (int t = 0; t < nt; t++)
            th.emplace_back([this] {
                int seen = 0;
                for (;;) {
                    { std::unique_lock<std::mutex> l(m); cv_go.wait(l, [&] { return quit || gen != seen; }); if (quit) return; seen = gen; }
                    for (int i; (i = next.fetch_add(1)) < n;) (*fn)(i);
                    { std::lock_guard<std::mutex> l(m); busy--; }
                    cv_done.notify_one();
                }
            });
    }
    ~BAHostPool() { { std::lock_guard<std::mutex> l(m); quit = true; } cv_go.notify_all(); for (auto &t : th) t.join(); }
    void run(int count, const std::function<void(int)> &f)              // f(0 .. count-1); the caller takes part
    {
        if (th.empty() || count <= 1) { for (int i = 0; i < count; i++) f(i); return; }
        { std::lock_guard<std::mutex> l(m); fn = &f; n = count; next.store(0); busy = (int)th.size(); gen++; }
        cv_go.notify_all();
        for (int i; (i = next.fetch_add(1)) < count;) f(i);
        std::unique_lock<std::mutex> l(m); cv_done.wait(l, [&] { return busy == 0; });
    }
};

static BAHostPool *ba_host_pool_of(ov2_ctx *ctx)
{
    if (!ctx->ba_host_pool) {
        try { ctx->ba_host_pool = new BAHostPool(15); }               // (no threads to be had: the caller works serially)
        catch (...) { ctx->ba_host_pool = nullptr; }
        ctx->ba_host_pool_free = [](void *q) { delete (BAHostPool *)q; };
    }
    return (BAHostPool *)ctx->ba_host_pool;
}

// transient: the problem lives for one ov2_ba_solve call -- small pools then come out of the context's device scratch instead of
// a hipMalloc / hipFree pair (~100 us, more than a whole ceresPnP solve)
static int ba_create(ov2_ctx *ctx, const ov2_ba_problem *p, ov2_ba_dev **out, bool transient = false, BASlice *ext = nullptr)
{
    OV2_REQUIRE(p && out, OV2_EINVAL, "NULL problem");
    OV2_REQUIRE(p->n_kf > 0 && p->n_lm >= 0 && p->n_res >= 0, OV2_EINVAL, "bad problem sizes");
    OV2_REQUIRE(p->poses && p->kf_const, OV2_EINVAL, "NULL pose arrays");
    OV2_REQUIRE(p->n_lm == 0 || (p->invdepth && p->lm_anchor_kf && p->lm_anchor_uv), OV2_EINVAL, "NULL landmark arrays");
    OV2_REQUIRE(p->n_res == 0 || (p->res_type && p->res_kf && p->res_lm && p->res_uv && p->res_sigma), OV2_EINVAL, "NULL residual arrays");
    // validate + landmark-sorted order of the active residual blocks (a STABLE counting sort: blocks of a landmark keep the
    // caller's order); pose-only blocks (OV2_RES_PNP) go to their own list.  Large problems (a 590 k-block localBA: 3.8 ms of the
    // call were this sort and the staging fill) split the residual range over a few host threads: per-thread counts, offsets
    // = landmark prefix + the counts of the lower-numbered threads, so the result is identical to the serial sort.
    // (a 25-KF window of 69 k blocks: 2 threads; the problems of a batch are prepared side by side already: one thread each)
    int NT = (p->n_res >= (1 << 16) && !ext) ? std::min(8, p->n_res >> 15) : 1;
    BAHostPool *hpool = NT > 1 ? ba_host_pool_of(ctx) : nullptr;
    if (!hpool) NT = 1;
    const BALap clap{"ba_create", ctx->debug != 0 && !ext};
    std::vector<std::vector<int>> cntT((size_t)NT, std::vector<int>((size_t)p->n_lm + 1, 0));
    std::vector<int> nactT((size_t)NT, 0), npoT((size_t)NT, 0);
    std::vector<const char *> errT((size_t)NT, nullptr);
    auto range_of = [&](int t, int &b, int &e) { b = (int)((long long)p->n_res * t / NT); e = (int)((long long)p->n_res * (t + 1) / NT); };
    auto run_threads = [&](auto &&fn) {
        if (NT == 1) { fn(0); return; }
        const std::function<void(int)> f = fn;                          // (the context's persistent threads: two spawns per call were 0.1 - 0.3 ms)
        hpool->run(NT, f);
    };
    run_threads([&](int t) {
        int b, e; range_of(t, b, e);
        std::vector<int> &cn = cntT[(size_t)t];
        int na_t = 0, np_t = 0;
        const char *err = nullptr;
        for (int i = b; i < e && !err; i++) {
            if (p->res_active && !p->res_active[i]) continue;
            if (p->res_type[i] > OV2_RES_PNP) { err = "unknown residual type"; break; }
            if (!(p->res_sigma[i] > 0)) { err = "res_sigma must be positive"; break; }
            if (p->res_type[i] == OV2_RES_PNP) {
                if (!p->res_xyz) { err = "OV2_RES_PNP blocks need res_xyz"; break; }
                if (p->res_kf[i] < 0 || p->res_kf[i] >= p->n_kf) { err = "res_kf out of range"; break; }
                np_t++;
                continue;
            }
            const int lm = p->res_lm[i];
            if (lm < 0 || lm >= p->n_lm) { err = "res_lm out of range"; break; }
            if (p->res_type[i] != OV2_RES_RIGHT_ANCH && (p->res_kf[i] < 0 || p->res_kf[i] >= p->n_kf)) { err = "res_kf out of range"; break; }
            // The observer of a LEFT / RIGHT block is never the landmark's anchor keyframe (the reference skips the anchor's own
            // mono observation, src/optimizer.cpp:290-296, and gives its right-camera observation the RIGHT_ANCH factor): the lineariser
            // relies on it (J_observer = -J_anchor serves both the observer's diagonal block and the anchor-observer block)
            if (p->res_type[i] != OV2_RES_RIGHT_ANCH && p->res_kf[i] == p->lm_anchor_kf[lm]) { err = "a LEFT / RIGHT block observes its landmark from the anchor keyframe (use OV2_RES_RIGHT_ANCH)"; break; }
            cn[lm]++; na_t++;
        }
        nactT[(size_t)t] = na_t; npoT[(size_t)t] = np_t; errT[(size_t)t] = err;
    });
    for (int t = 0; t < NT; t++) OV2_REQUIRE(errT[(size_t)t] == nullptr, OV2_EINVAL, errT[(size_t)t]);
    clap("validate + count");
    std::vector<int> cnt(p->n_lm + 1, 0);                              // cnt[l] = first sorted index of landmark l (CSR)
    int n_act = 0, n_po = 0;
    for (int t = 0; t < NT; t++) { n_act += nactT[(size_t)t]; n_po += npoT[(size_t)t]; }
    {
        int run = 0;
        for (int l = 0; l < p->n_lm; l++) {
            OV2_REQUIRE(p->lm_anchor_kf[l] >= 0 && p->lm_anchor_kf[l] < p->n_kf, OV2_EINVAL, "lm_anchor_kf out of range");
            cnt[l] = run;
            for (int t = 0; t < NT; t++) { const int c = cntT[(size_t)t][l]; cntT[(size_t)t][l] = run; run += c; }   // cntT becomes the thread's fill cursor
        }
        cnt[p->n_lm] = run;
    }
    std::vector<int> pose_col(p->n_kf);
    int n_opt = 0;
    for (int k = 0; k < p->n_kf; k++) pose_col[k] = p->kf_const[k] ? -1 : 6 * n_opt++;
    const int nf = 6 * n_opt, nfp = ba_nfp(n_opt);
    OV2_REQUIRE(nfp <= BA_MAX_NFP, OV2_EUNSUPPORTED, "more than 1024 optimised keyframes: dense reduced system too large");
    // the per-residual upload arrays are filled straight into the context's PINNED host scratch: the H2D copies below are then
    // real asynchronous DMA (from pageable std::vectors every copy went through the runtime's staging buffer, ~2.5 ms for the
    // 20 MB of a 590 k-block problem) and no 20 MB of vectors is allocated and zeroed per call
    int *res_kf, *res_orig, *po_kf, *po_orig;
    uint8_t *res_type;
    double *res_uv, *res_sigma, *po_xyz, *po_uv, *po_sigma;
    // Round 3: the staging buffer MIRRORS the first eleven arrays of the device pool (same offsets), so that everything a solve
    // needs from the host goes up in ONE copy instead of eleven (each ~15 us of launch overhead: a third of ba_create on a
    // 69 k-block window)
    const size_t nl = (size_t)std::max(1, p->n_lm), na = (size_t)std::max(1, n_act), nr = (size_t)std::max(1, p->n_res);
    StageCursor c(256);
    const size_t o_pose_col = c.take(4 * (size_t)p->n_kf), o_lm_ptr = c.take(4 * (nl + 1)), o_lm_anchor = c.take(4 * nl), o_lm_auv = c.take(16 * nl);
    const size_t o_res_type = c.take(na), o_res_kf = c.take(4 * na), o_res_orig = c.take(4 * na), o_res_uv = c.take(16 * na), o_res_sigma = c.take(8 * na);
    const size_t o_lm_order = c.take(4 * nl), o_lm_live = c.take(nl);
    const size_t o_pose0 = c.take(56 * (size_t)p->n_kf), o_lam0 = c.take(8 * nl);      // initial parameters (the batch's reset kernel copies them on the device)
    const size_t up_bytes = c.off;                                       // [0, up_bytes) of the pool = the staging buffer
    uint8_t *hs = nullptr;
    {
        const size_t np_h = (size_t)std::max(1, n_po);
        StageCursor hc = c;                                            // the host block goes on behind the staging buffer with sections of its own
        const size_t h6 = hc.take(4 * np_h), h7 = hc.take(4 * np_h), h8 = hc.take(24 * np_h), h9 = hc.take(16 * np_h), h10 = hc.take(8 * np_h);
        if (ext) {
            std::lock_guard<std::mutex> l(ext->m);
            if (ext->host_used + hc.off > ext->host_cap) { ext->host_used += hc.off; return BA_SLICE_FULL; }    // (keeps counting: the caller learns the total)
            hs = ext->host_base + ext->host_used; ext->host_used += hc.off;
        } else {
        const int rch = ctx->reserve_host(hc.off);
        if (rch != OV2_OK) return rch;
        hs = (uint8_t *)ctx->h_scratch;
        }
        res_kf = (int *)(hs + o_res_kf); res_orig = (int *)(hs + o_res_orig); res_type = hs + o_res_type; res_uv = (double *)(hs + o_res_uv); res_sigma = (double *)(hs + o_res_sigma);
        po_kf = (int *)(hs + h6); po_orig = (int *)(hs + h7); po_xyz = (double *)(hs + h8); po_uv = (double *)(hs + h9); po_sigma = (double *)(hs + h10);
    }
    std::vector<int> poStart((size_t)NT + 1, 0);
    for (int t = 0; t < NT; t++) poStart[(size_t)t + 1] = poStart[(size_t)t] + npoT[(size_t)t];
    run_threads([&](int t) {
        int b, e; range_of(t, b, e);
        std::vector<int> &fill = cntT[(size_t)t];
        int kp = poStart[(size_t)t];
        for (int i = b; i < e; i++) {
            if (p->res_active && !p->res_active[i]) continue;
            if (p->res_type[i] == OV2_RES_PNP) {
                po_kf[kp] = p->res_kf[i]; po_orig[kp] = i; po_sigma[kp] = p->res_sigma[i];
                po_uv[2 * kp] = p->res_uv[2 * i]; po_uv[2 * kp + 1] = p->res_uv[2 * i + 1];
                for (int c = 0; c < 3; c++) po_xyz[3 * kp + c] = p->res_xyz[3 * i + c];
                kp++;
                continue;
            }
            const int k = fill[p->res_lm[i]]++;
            res_type[k] = p->res_type[i]; res_kf[k] = p->res_type[i] == OV2_RES_RIGHT_ANCH ? p->lm_anchor_kf[p->res_lm[i]] : p->res_kf[i];
            res_orig[k] = i; res_uv[2 * k] = p->res_uv[2 * i]; res_uv[2 * k + 1] = p->res_uv[2 * i + 1]; res_sigma[k] = p->res_sigma[i];
        }
    });

    clap("fill staging (sorted blocks)");
    OV2_HIP_CHECK(hipSetDevice(ctx->device));
    ov2_ba_dev *dev = new (std::nothrow) ov2_ba_dev();
    OV2_REQUIRE(dev != nullptr, OV2_ENOMEM, "out of host memory");
    dev->device = ctx->device; dev->n_res = p->n_res;
    if (!ext) dev->h_poses0.assign(p->poses, p->poses + 7 * (size_t)p->n_kf);
    if (!ext) dev->h_lam0.assign(p->invdepth, p->invdepth + (p->n_lm > 0 ? p->n_lm : 0));
    BADev &D = dev->D;
    memset(&D, 0, sizeof(D));
    D.n_kf = p->n_kf; D.n_lm = p->n_lm; D.n_act = n_act; D.nf = nf; D.nfp = nfp; D.n_po = n_po; D.ldim = 1; D.n_res = p->n_res;
    // beyond what the LDS-resident lineariser / Cholesky hold (69 optimised keyframes): sparse W + HBM Cholesky (BADev::big); from 583
    // the big-path linearisers cannot pre-aggregate the observer blocks in LDS either.  The decisions are ba_geom.hpp's.
    D.big = !ba_small_path(n_opt) || ctx->ba_force_large;                      // OV2_OPT_BA_FORCE_LARGE: the path on small problems (tests)
    D.lin_direct = D.big && (ba_lin_direct(n_opt) || ctx->ba_lin_direct);      // OV2_OPT_BA_LIN_DIRECT (tests: force it on small problems)
    D.chol_hbm = D.big; D.lin_waves = 4;
    // big path: the slots of the sparse W (one per landmark and optimised keyframe seeing or anchoring it) and their per-keyframe lists
    std::vector<int> cw_ptr(p->n_lm + 1, 0), cw_col, cw_lm, res_cw, lm_cwa, kfl_ptr(n_opt + 1, 0), kfl_idx;
    if (D.big) {
        res_cw.assign(std::max(1, n_act), -1); lm_cwa.assign(std::max(1, p->n_lm), -1);
        std::vector<int> slot_of(std::max(1, n_opt), -1), touched;
        for (int l = 0; l < p->n_lm; l++) {
            cw_ptr[l] = (int)cw_col.size();
            touched.clear();
            auto get = [&](int col) {
                const int ob = col / 6;
                if (slot_of[ob] < 0) { slot_of[ob] = (int)cw_col.size(); cw_col.push_back(col); cw_lm.push_back(l); touched.push_back(ob); }
                return slot_of[ob];
            };
            if (cnt[l] != cnt[l + 1]) {
                const int ca = pose_col[p->lm_anchor_kf[l]];
                if (ca >= 0) lm_cwa[l] = get(ca);
                for (int k = cnt[l]; k < cnt[l + 1]; k++) {
                    if (res_type[k] == OV2_RES_RIGHT_ANCH) continue;
                    const int co = pose_col[res_kf[k]];
                    if (co >= 0) res_cw[k] = get(co);
                }
            }
            for (int ob : touched) slot_of[ob] = -1;
        }
        cw_ptr[p->n_lm] = (int)cw_col.size();
        for (int c : cw_col) kfl_ptr[c / 6 + 1]++;
        for (int k = 0; k < n_opt; k++) kfl_ptr[k + 1] += kfl_ptr[k];
        kfl_idx.resize(cw_col.size());
        std::vector<int> kfill(kfl_ptr.begin(), kfl_ptr.end() - 1);
        for (size_t j = 0; j < cw_col.size(); j++) kfl_idx[kfill[cw_col[j] / 6]++] = (int)j;
    }
    D.n_cw = (int)cw_col.size();
    const size_t ncw = (size_t)std::max(1, D.n_cw);
    const size_t o_x_pose = c.take(56 * (size_t)p->n_kf), o_c_pose = c.take(56 * (size_t)p->n_kf), o_x_RT = c.take(96 * (size_t)p->n_kf), o_c_RT = c.take(96 * (size_t)p->n_kf);
    const size_t o_x_lam = c.take(8 * nl), o_c_lam = c.take(8 * nl), o_scale_f = c.take(8 * (size_t)nfp), o_diag_f = c.take(8 * (size_t)nfp);
    const size_t o_scale_l = c.take(8 * nl), o_diag_l = c.take(8 * nl), o_ete = c.take(8 * nl), o_etb = c.take(8 * nl), o_cl = c.take(8 * nl), o_ce = c.take(8 * nl);
    const size_t o_W = c.take(D.big ? 256 : 8 * nl * nfp), o_H = c.take(8 * (size_t)nfp * nfp), o_G = c.take(8 * (size_t)nfp * nfp), o_S = c.take(8 * (size_t)nfp * nfp);
    const size_t o_cww = c.take(48 * ncw), o_cw_ptr = c.take(4 * (nl + 1)), o_cw_col = c.take(4 * ncw), o_cw_lm = c.take(4 * ncw);
    const size_t o_res_cw = c.take(4 * na), o_lm_cwa = c.take(4 * nl), o_kfl_ptr = c.take(4 * ((size_t)n_opt + 1)), o_kfl_idx = c.take(4 * ncw);
    const size_t o_bf = c.take(8 * (size_t)nfp), o_v = c.take(8 * (size_t)nfp), o_yf = c.take(8 * (size_t)nfp), o_yl = c.take(8 * nl);
    const size_t o_Linv = c.take(8 * (size_t)nfp * 32);
    const size_t o_chi2 = c.take(8 * nr), o_dpos = c.take(nr), o_ctl = c.take(sizeof(BACtl));
    const size_t o_res_off = c.take(na), o_bad_obs = c.take(nr), o_lba_cnt = c.take(64), o_part = c.take(8 * 7 * BA_PART_MAX);
    const size_t npo = (size_t)std::max(1, n_po);
    const size_t o_po_kf = c.take(4 * npo), o_po_orig = c.take(4 * npo), o_po_xyz = c.take(24 * npo), o_po_uv = c.take(16 * npo), o_po_sigma = c.take(8 * npo);
    dev->pool_bytes = c.off;
    if (ext) {
        std::lock_guard<std::mutex> l(ext->m);
        if (ext->dev_used + c.off > ext->dev_cap) { ext->dev_used += up256(c.off); delete dev; return BA_SLICE_FULL; }
        dev->pool = ext->dev_base + ext->dev_used; dev->pool_owned = false; ext->dev_used += up256(c.off);
    } else if (transient && c.off <= ((size_t)64 << 20)) {               // (the context keeps the largest pool it has seen: grow-only scratch)
        const int rcs = ctx->reserve_device(c.off);
        if (rcs != OV2_OK) { delete dev; return rcs; }
        dev->pool = ctx->d_scratch; dev->pool_owned = false;
    } else {
        hipError_t e = hipMalloc(&dev->pool, dev->pool_bytes);
        if (e != hipSuccess) { delete dev; ov2_set_error("hipMalloc(%zu): %s", c.off, hipGetErrorString(e)); return OV2_ENOMEM; }
    }
    uint8_t *b = (uint8_t *)dev->pool;
    D.pose_col = (int *)(b + o_pose_col); D.lm_ptr = (int *)(b + o_lm_ptr); D.lm_anchor = (int *)(b + o_lm_anchor); D.lm_auv = (double *)(b + o_lm_auv);
    D.res_type = b + o_res_type; D.res_kf = (int *)(b + o_res_kf); D.res_orig = (int *)(b + o_res_orig); D.res_uv = (double *)(b + o_res_uv); D.res_sigma = (double *)(b + o_res_sigma);
    D.x_pose = (double *)(b + o_x_pose); D.c_pose = (double *)(b + o_c_pose); D.x_RT = (double *)(b + o_x_RT); D.c_RT = (double *)(b + o_c_RT);
    D.x_lam = (double *)(b + o_x_lam); D.c_lam = (double *)(b + o_c_lam); D.scale_f = (double *)(b + o_scale_f); D.diag_f = (double *)(b + o_diag_f);
    D.scale_l = (double *)(b + o_scale_l); D.diag_l = (double *)(b + o_diag_l); D.ete = (double *)(b + o_ete); D.etb = (double *)(b + o_etb);
    D.part = (double *)(b + o_part);
    D.cl = (double *)(b + o_cl); D.ce = (double *)(b + o_ce); D.W = (double *)(b + o_W); D.H = (double *)(b + o_H); D.G = (double *)(b + o_G); D.S = (double *)(b + o_S);
    D.Linv = (double *)(b + o_Linv);
    D.cww = (double *)(b + o_cww); D.cw_ptr = (int *)(b + o_cw_ptr); D.cw_col = (int *)(b + o_cw_col); D.cw_lm = (int *)(b + o_cw_lm);
    D.res_cw = (int *)(b + o_res_cw); D.lm_cwa = (int *)(b + o_lm_cwa); D.kfl_ptr = (int *)(b + o_kfl_ptr); D.kfl_idx = (int *)(b + o_kfl_idx);
    D.bf = (double *)(b + o_bf); D.v = (double *)(b + o_v); D.yf = (double *)(b + o_yf); D.yl = (double *)(b + o_yl);
    D.chi2 = (double *)(b + o_chi2); D.dpos = b + o_dpos; D.ctl = (BACtl *)(b + o_ctl);
    dev->lm_order = (int *)(b + o_lm_order);
    D.lm_order_b = dev->lm_order; D.pose0 = (const double *)(b + o_pose0); D.lam0 = (const double *)(b + o_lam0);
    D.res_off = b + o_res_off; D.lm_live = b + o_lm_live; D.bad_obs = b + o_bad_obs; D.lba_cnt = (int *)(b + o_lba_cnt);
    D.po_kf = (int *)(b + o_po_kf); D.po_orig = (int *)(b + o_po_orig); D.po_xyz = (double *)(b + o_po_xyz); D.po_uv = (double *)(b + o_po_uv); D.po_sigma = (double *)(b + o_po_sigma);
    for (int i = 0; i < 4; i++) { D.calib_l[i] = p->calib_l[i]; D.calib_r[i] = p->calib_r[i]; }
    ba_set_extrinsic(D, p->T_rl);
    hipStream_t s = ctx->stream;
    {   // the small arrays join the residual arrays in the staging mirror; landmarks are processed anchor by anchor (lm_order)
        int *lm_order = (int *)(hs + o_lm_order);
        {   // stable counting sort by anchor keyframe (a std::stable_sort of 3000 landmarks was 60 us of a 0.45 ms call)
            std::vector<int> first((size_t)p->n_kf + 1, 0);
            for (int l = 0; l < p->n_lm; l++) first[(size_t)p->lm_anchor_kf[l] + 1]++;
            for (int k = 0; k < p->n_kf; k++) first[(size_t)k + 1] += first[(size_t)k];
            for (int l = 0; l < p->n_lm; l++) lm_order[first[(size_t)p->lm_anchor_kf[l]]++] = l;
        }
        uint8_t *lm_live = hs + o_lm_live;
        for (int l = 0; l < p->n_lm; l++) lm_live[l] = cnt[l] != cnt[l + 1];
        memcpy(hs + o_pose_col, pose_col.data(), 4 * (size_t)p->n_kf);
        memcpy(hs + o_lm_ptr, cnt.data(), 4 * ((size_t)p->n_lm + 1));
        if (p->n_lm > 0) { memcpy(hs + o_lm_anchor, p->lm_anchor_kf, 4 * (size_t)p->n_lm); memcpy(hs + o_lm_auv, p->lm_anchor_uv, 16 * (size_t)p->n_lm); }
        memcpy(hs + o_pose0, p->poses, 56 * (size_t)p->n_kf);
        if (p->n_lm > 0) memcpy(hs + o_lam0, p->invdepth, 8 * (size_t)p->n_lm);
    }
    clap("views + small arrays + lm_order");
    BA_UP(b, hs, up_bytes);                                               // ONE copy: pose_col .. lam0
    if (!ext) {                                                        // (batch: k_ba_reset_B clears them)
        hipError_t em = hipMemsetAsync(D.res_off, 0, na, s);
        if (em == hipSuccess) em = hipMemsetAsync(D.bad_obs, 0, nr, s);
        if (em == hipSuccess) em = hipMemsetAsync(D.lba_cnt, 0, 64, s);
        if (em != hipSuccess) { ov2_set_error("hipMemsetAsync: %s", hipGetErrorString(em)); ba_destroy(dev); return OV2_EHIP; }
    }
    BA_UP(D.po_kf, po_kf, 4 * (size_t)n_po); BA_UP(D.po_orig, po_orig, 4 * (size_t)n_po);
    BA_UP(D.po_xyz, po_xyz, 24 * (size_t)n_po); BA_UP(D.po_uv, po_uv, 16 * (size_t)n_po); BA_UP(D.po_sigma, po_sigma, 8 * (size_t)n_po);
    if (D.big) {
        BA_UP(D.cw_ptr, cw_ptr.data(), 4 * ((size_t)p->n_lm + 1)); BA_UP(D.cw_col, cw_col.data(), 4 * (size_t)D.n_cw); BA_UP(D.cw_lm, cw_lm.data(), 4 * (size_t)D.n_cw);
        BA_UP(D.res_cw, res_cw.data(), 4 * (size_t)n_act); BA_UP(D.lm_cwa, lm_cwa.data(), 4 * (size_t)p->n_lm);
        BA_UP(D.kfl_ptr, kfl_ptr.data(), 4 * ((size_t)n_opt + 1)); BA_UP(D.kfl_idx, kfl_idx.data(), 4 * (size_t)D.n_cw);
    }
    // the staging vectors die at return: make sure the copies are done (a batch slice's staging lives until the batch is through)
    if (!ext || D.big) {
        const hipError_t es = hipStreamSynchronize(s);
        if (es != hipSuccess) { ov2_set_error("hipStreamSynchronize: %s", hipGetErrorString(es)); ba_destroy(dev); return OV2_EHIP; }
    }
    clap("upload enqueued + synchronised");
    *out = dev;
    return OV2_OK;
}

// 3-D point landmarks with variable poses (ldim = 3): same device object, point-sorted residual blocks
static int xyzba_create(ov2_ctx *ctx, const ov2_xyzba_problem *p, ov2_ba_dev **out)
{
    OV2_REQUIRE(p && out, OV2_EINVAL, "NULL problem");
    OV2_REQUIRE(p->n_kf > 0 && p->n_pts >= 0 && p->n_res >= 0, OV2_EINVAL, "bad problem sizes");
    OV2_REQUIRE(p->poses, OV2_EINVAL, "NULL pose array");
    OV2_REQUIRE(p->n_pts == 0 || p->xyz, OV2_EINVAL, "NULL point array");
    OV2_REQUIRE(p->n_res == 0 || (p->res_type && p->res_kf && p->res_pt && p->res_uv && p->res_sigma), OV2_EINVAL, "NULL residual arrays");
    std::vector<int> cnt(p->n_pts + 1, 0);
    int n_act = 0;
    for (int i = 0; i < p->n_res; i++) {
        if (p->res_active && !p->res_active[i]) continue;
        OV2_REQUIRE(p->res_type[i] <= OV2_XYZ_RIGHT, OV2_EINVAL, "unknown residual type");
        OV2_REQUIRE(p->res_sigma[i] > 0, OV2_EINVAL, "res_sigma must be positive");
        OV2_REQUIRE(p->res_pt[i] >= 0 && p->res_pt[i] < p->n_pts, OV2_EINVAL, "res_pt out of range");
        OV2_REQUIRE(p->res_kf[i] >= 0 && p->res_kf[i] < p->n_kf, OV2_EINVAL, "res_kf out of range");
        cnt[p->res_pt[i] + 1]++; n_act++;
    }
    for (int l = 0; l < p->n_pts; l++) cnt[l + 1] += cnt[l];
    std::vector<int> pose_col(p->n_kf);
    int n_opt = 0;
    for (int k = 0; k < p->n_kf; k++) pose_col[k] = (p->kf_const && p->kf_const[k]) ? -1 : 6 * n_opt++;
    const int nf = 6 * n_opt, nfp = ba_nfp(n_opt);
    // Size limits BEFORE anything is allocated or uploaded (W and W' alone are 2 x 24 n_pts nfp bytes).  The 3-D point form keeps
    // W dense: its lineariser holds 3 rows of it per wavefront in LDS next to the observer blocks (4 wavefronts per work-group up
    // to 202 optimised keyframes, then 2 up to 320, then 1 up to 451: ba_xyz_lin_waves), and beyond 69 keyframes the reduced system is
    // factored by the multi-kernel Cholesky on HBM instead of the one-work-group LDS kernel (ba_chol_hbm).
    int lin_waves = ba_xyz_lin_waves(n_opt, nfp);
    if (ctx->ba_xyz_lin_waves == 1 || ctx->ba_xyz_lin_waves == 2) lin_waves = lin_waves ? std::min(lin_waves, ctx->ba_xyz_lin_waves) : 0;   // OV2_OPT_BA_XYZ_LIN_WAVES (tests)
    if (!lin_waves || nfp > BA_MAX_NFP) {
        ov2_set_error("too many optimised keyframes (%d) for the 3-D point form (limit 451: dense W rows in LDS)", n_opt);
        return OV2_EUNSUPPORTED;
    }
    const int chol_hbm = ba_chol_hbm(n_opt, nfp) || ctx->ba_force_large;         // OV2_OPT_BA_FORCE_LARGE (tests: the HBM factorisation on small problems)
    std::vector<int> fill(cnt.begin(), cnt.end() - 1), res_kf(n_act), res_orig(n_act);
    std::vector<uint8_t> res_type(n_act);
    std::vector<double> res_uv(2 * (size_t)n_act), res_sigma(n_act);
    for (int i = 0; i < p->n_res; i++) {
        if (p->res_active && !p->res_active[i]) continue;
        const int k = fill[p->res_pt[i]]++;
        res_type[k] = p->res_type[i]; res_kf[k] = p->res_kf[i]; res_orig[k] = i;
        res_uv[2 * k] = p->res_uv[2 * i]; res_uv[2 * k + 1] = p->res_uv[2 * i + 1]; res_sigma[k] = p->res_sigma[i];
    }
    OV2_HIP_CHECK(hipSetDevice(ctx->device));
    ov2_ba_dev *dev = new (std::nothrow) ov2_ba_dev();
    OV2_REQUIRE(dev != nullptr, OV2_ENOMEM, "out of host memory");
    dev->device = ctx->device; dev->n_res = p->n_res;
    dev->h_poses0.assign(p->poses, p->poses + 7 * (size_t)p->n_kf);
    dev->h_lam0.assign(p->xyz, p->xyz + 3 * (size_t)(p->n_pts > 0 ? p->n_pts : 0));
    BADev &D = dev->D;
    memset(&D, 0, sizeof(D));
    D.n_kf = p->n_kf; D.n_lm = p->n_pts; D.n_act = n_act; D.nf = nf; D.nfp = nfp; D.n_po = 0; D.ldim = 3;
    D.chol_hbm = chol_hbm; D.lin_waves = lin_waves;
    const size_t nl = (size_t)std::max(1, p->n_pts), na = (size_t)std::max(1, n_act), nr = (size_t)std::max(1, p->n_res);
    StageCursor c(256);
    const size_t o_pose_col = c.take(4 * (size_t)p->n_kf), o_lm_ptr = c.take(4 * (nl + 1));
    const size_t o_res_type = c.take(na), o_res_kf = c.take(4 * na), o_res_orig = c.take(4 * na), o_res_uv = c.take(16 * na), o_res_sigma = c.take(8 * na);
    const size_t o_x_pose = c.take(56 * (size_t)p->n_kf), o_c_pose = c.take(56 * (size_t)p->n_kf), o_x_RT = c.take(96 * (size_t)p->n_kf), o_c_RT = c.take(96 * (size_t)p->n_kf);
    const size_t o_x_lam = c.take(24 * nl), o_c_lam = c.take(24 * nl), o_scale_f = c.take(8 * (size_t)nfp), o_diag_f = c.take(8 * (size_t)nfp);
    const size_t o_scale_l = c.take(24 * nl), o_diag_l = c.take(24 * nl), o_etb = c.take(24 * nl), o_yl = c.take(24 * nl), o_ep = c.take(24 * nl), o_ones = c.take(24 * nl);
    const size_t o_ete6 = c.take(48 * nl), o_minv6 = c.take(48 * nl);
    const size_t o_W = c.take(24 * nl * nfp), o_Wp = c.take(24 * nl * nfp);
    const size_t o_H = c.take(8 * (size_t)nfp * nfp), o_G = c.take(8 * (size_t)nfp * nfp), o_S = c.take(8 * (size_t)nfp * nfp);
    const size_t o_bf = c.take(8 * (size_t)nfp), o_v = c.take(8 * (size_t)nfp), o_yf = c.take(8 * (size_t)nfp), o_Linv = c.take(8 * (size_t)nfp * 32);
    const size_t o_chi2 = c.take(8 * nr), o_dpos = c.take(nr), o_ctl = c.take(sizeof(BACtl));
    dev->pool_bytes = c.off;
    hipError_t e = hipMalloc(&dev->pool, dev->pool_bytes);
    if (e != hipSuccess) { delete dev; ov2_set_error("hipMalloc(%zu): %s", c.off, hipGetErrorString(e)); return OV2_ENOMEM; }
    uint8_t *b = (uint8_t *)dev->pool;
    D.pose_col = (int *)(b + o_pose_col); D.lm_ptr = (int *)(b + o_lm_ptr);
    D.res_type = b + o_res_type; D.res_kf = (int *)(b + o_res_kf); D.res_orig = (int *)(b + o_res_orig); D.res_uv = (double *)(b + o_res_uv); D.res_sigma = (double *)(b + o_res_sigma);
    D.x_pose = (double *)(b + o_x_pose); D.c_pose = (double *)(b + o_c_pose); D.x_RT = (double *)(b + o_x_RT); D.c_RT = (double *)(b + o_c_RT);
    D.x_lam = (double *)(b + o_x_lam); D.c_lam = (double *)(b + o_c_lam); D.scale_f = (double *)(b + o_scale_f); D.diag_f = (double *)(b + o_diag_f);
    D.scale_l = (double *)(b + o_scale_l); D.diag_l = (double *)(b + o_diag_l); D.etb = (double *)(b + o_etb); D.yl = (double *)(b + o_yl);
    D.ep = (double *)(b + o_ep); D.ones = (double *)(b + o_ones); D.ete6 = (double *)(b + o_ete6); D.minv6 = (double *)(b + o_minv6);
    D.W = (double *)(b + o_W); D.Wp = (double *)(b + o_Wp); D.H = (double *)(b + o_H); D.G = (double *)(b + o_G); D.S = (double *)(b + o_S);
    D.bf = (double *)(b + o_bf); D.v = (double *)(b + o_v); D.yf = (double *)(b + o_yf); D.Linv = (double *)(b + o_Linv);
    D.chi2 = (double *)(b + o_chi2); D.dpos = b + o_dpos; D.ctl = (BACtl *)(b + o_ctl);
    D.cl = D.ones; D.ce = D.ep; D.ete = D.ete6;              // (scalar-landmark views, unused when ldim == 3)
    for (int i = 0; i < 4; i++) { D.calib_l[i] = p->calib_l[i]; D.calib_r[i] = p->calib_r[i]; }
    ba_set_extrinsic(D, p->T_rl);
    hipStream_t s = ctx->stream;
    BA_UP(D.pose_col, pose_col.data(), 4 * (size_t)p->n_kf);
    BA_UP(D.lm_ptr, cnt.data(), 4 * ((size_t)p->n_pts + 1));
    BA_UP(D.res_type, res_type.data(), (size_t)n_act);
    BA_UP(D.res_kf, res_kf.data(), 4 * (size_t)n_act);
    BA_UP(D.res_orig, res_orig.data(), 4 * (size_t)n_act);
    BA_UP(D.res_uv, res_uv.data(), 16 * (size_t)n_act);
    BA_UP(D.res_sigma, res_sigma.data(), 8 * (size_t)n_act);
    {
        const hipError_t es = hipStreamSynchronize(s);
        if (es != hipSuccess) { ov2_set_error("hipStreamSynchronize: %s", hipGetErrorString(es)); ba_destroy(dev); return OV2_EHIP; }
    }
    *out = dev;
    return OV2_OK;
}

static void ba_destroy(ov2_ba_dev *dev)
{
    if (!dev) return;
    (void)hipSetDevice(dev->device);
    if (dev->pool && dev->pool_owned) (void)hipFree(dev->pool);
    delete dev;
}

