// ba_chol.hpp -- the factorisation of the reduced camera system: the one-work-group LDS-panel Cholesky (k_ba_cholesky) and the
// blocked multi-kernel Cholesky on HBM (k_chol_*) for systems that outgrow it.  A part of ba.hip (same translation unit):
// included there after BADev / BACtl and under that file's floating-point mode.
#pragma once

// ---------------------------------------------------------------------------------- reduced system (1 block)
// S = s_i s_j (H_ij - G_ij) + delta_ij diag_i / radius ; rhs = s_i (b_i - v_i); blocked Cholesky; solve.
// Right-looking, 32-wide panels: the diagonal block is factored in LDS by one wavefront, the panel
// below it is solved row-per-thread against that block and parked in LDS, and the trailing update
// reads the panel from LDS only (each S entry is touched once per panel).
// (CH_NB, CH_LDP, CH_MAX_LDS_N and the kernels' dynamic-LDS sizes, chol_lds_bytes / chol_solve_lds_bytes: ba_geom.hpp)
#define CH_GRP 8           // columns of the diagonal block published per work-group barrier (pipelined panel solve): 2 / 4 / 8 -> 102 / 89 / 87 us
// knock-out timings of k_ba_cholesky's phases (no MFMA, no loads of the old tile values, no tile stores, no LDS operand reads, a
// quarter of the panel solve's terms): profiles/archive/r4_ba_dead_ends.txt

// The two triangular solves L y = rhs, L^T x = y on the factor in S (HBM) with the inverse diagonal blocks in Linv; yv (LDS, nfp
// doubles) holds rhs on entry and x on return, L11 is a CH_NB x CH_LDP LDS scratch.  One work-group.
__device__ __forceinline__ void chol_trisolve(const BADev &D, double *L11, double *yv, double (*s_red)[33], bool forward_done = false)
{
    const int n = D.nf, ld = D.nfp, tid = threadIdx.x, nt = blockDim.x;
    const double *S = D.S, *Linv = D.Linv;
    // forward substitution  L y = rhs, left-looking by blocks:  y_blk = Linv_blk (b_blk - L[blk, 0:k0] y[0:k0])
    // (forward_done: yv already holds y -- k_ba_cholesky carries the right-hand side through the factorisation as one more panel row)
    const int tr = tid >> 5, tcn = tid & 31, ngr = nt >> 5;  // ngr groups of 32 partial-sum threads
    for (int k0 = 0; k0 < n && !forward_done; k0 += CH_NB) {
        const int nb = min(CH_NB, n - k0);
        for (int r = tr; r < CH_NB; r += ngr) {
            double part = 0;
            if (r < nb) for (int k = tcn; k < k0; k += 32) part += S[(long long)(k0 + r) * ld + k] * yv[k];
            s_red[r][tcn] = part;
        }
        for (int e = tid; e < CH_NB * CH_NB; e += nt) L11[(e >> 5) * CH_LDP + (e & 31)] = Linv[(long long)(k0 / CH_NB) * CH_NB * CH_NB + e];
        __syncthreads();
        if (tid < CH_NB) {
            double r = 0;
            for (int q = 0; q < 32; q++) r += s_red[tid][q];
            s_red[tid][32] = tid < nb ? yv[k0 + tid] - r : 0.0;
        }
        __syncthreads();
        if (tid < nb) {
            double r = 0;
            for (int k = 0; k <= tid; k++) r += L11[tid * CH_LDP + k] * s_red[k][32];
            yv[k0 + tid] = r;
        }
        __syncthreads();
    }
    // backward substitution  L^T x = y, right-looking by blocks, last block first:  x_blk = Linv_blk^T y_blk, then
    // y[0:k0] -= L[blk, 0:k0]^T x_blk.  Nothing the loop loads depends on x: thread t keeps column t of the block row L[blk, 0:k0]
    // (32 doubles, coalesced over t) and its share of Linv_blk in registers, requested one block ahead, so that a block costs two
    // barriers and 2 x 32 FMAs instead of a dependent walk over L in L2 with three barriers (round 4: 44 -> ~12 us at n = 300).
    if (n <= nt && nt >= 256) {
        const int nblk = (n + CH_NB - 1) / CH_NB;
        constexpr int NINV = CH_NB * CH_NB / 256;                // Linv doubles per thread at the smallest work-group (256)
        double cur[CH_NB], nxt[CH_NB], winv[NINV], ninv[NINV];
        auto load_rows = [&](int k0, int nb, double (&v)[CH_NB]) {
#pragma unroll
            for (int i = 0; i < CH_NB; i++) v[i] = (tid < k0 && i < nb) ? S[(long long)(k0 + i) * ld + tid] : 0.0;
        };
        auto load_inv = [&](int blk, double (&w)[NINV]) {
#pragma unroll
            for (int u = 0; u < NINV; u++) { const int e = tid + u * nt; w[u] = e < CH_NB * CH_NB ? Linv[(long long)blk * CH_NB * CH_NB + e] : 0.0; }
        };
        load_rows((nblk - 1) * CH_NB, n - (nblk - 1) * CH_NB, cur);
        load_inv(nblk - 1, winv);
        for (int blk = nblk - 1; blk >= 0; blk--) {
            const int k0 = blk * CH_NB, nb = min(CH_NB, n - k0);
#pragma unroll
            for (int u = 0; u < NINV; u++) { const int e = tid + u * nt; if (e < CH_NB * CH_NB) L11[(e >> 5) * CH_LDP + (e & 31)] = winv[u]; }
            if (blk > 0) { load_rows(k0 - CH_NB, CH_NB, nxt); load_inv(blk - 1, ninv); }
            __syncthreads();                                     // the inverse block is staged, y carries every later block's update
            if (tid < CH_NB) {
                double r = 0;
                for (int k = tid; k < nb; k++) r += L11[k * CH_LDP + tid] * yv[k0 + k];     // Linv^T
                s_red[tid][32] = tid < nb ? r : 0.0;
            }
            __syncthreads();
            if (tid < nb) yv[k0 + tid] = s_red[tid][32];
            if (tid < k0) {
                double acc = yv[tid];
#pragma unroll
                for (int i = 0; i < CH_NB; i++) acc -= cur[i] * s_red[i][32];
                yv[tid] = acc;
            }
#pragma unroll
            for (int i = 0; i < CH_NB; i++) cur[i] = nxt[i];
#pragma unroll
            for (int u = 0; u < NINV; u++) winv[u] = ninv[u];
        }
        __syncthreads();
        return;
    }
    // (systems wider than the work-group: the large-problem path) left-looking, x_blk = Linv_blk^T (y_blk - L[below, blk]^T x[below])
    for (int k0 = ((n - 1) / CH_NB) * CH_NB; k0 >= 0; k0 -= CH_NB) {
        const int nb = min(CH_NB, n - k0);
        // lanes along the block's columns (coalesced), thread groups along the rows below
        for (int g = tr; g < 32; g += ngr) {
            double part = 0;
            if (tcn < nb) for (int i = k0 + nb + g; i < n; i += 32) part += S[(long long)i * ld + k0 + tcn] * yv[i];
            s_red[tcn][g] = part;
        }
        for (int e = tid; e < CH_NB * CH_NB; e += nt) L11[(e >> 5) * CH_LDP + (e & 31)] = Linv[(long long)(k0 / CH_NB) * CH_NB * CH_NB + e];
        __syncthreads();
        if (tid < CH_NB) {
            double r = 0;
            for (int q = 0; q < 32; q++) r += s_red[tid][q];
            s_red[tid][32] = tid < nb ? yv[k0 + tid] - r : 0.0;
        }
        __syncthreads();
        if (tid < nb) {
            double r = 0;
            for (int k = tid; k < nb; k++) r += L11[k * CH_LDP + tid] * s_red[k][32];     // Linv^T
            yv[k0 + tid] = r;
        }
        __syncthreads();
    }
}

// Backward substitution  L^T x = y  on the factor in S WITHOUT inverse diagonal blocks (k_ba_cholesky, round 4): right-looking by
// blocks, last block first.  Wavefront 0 solves the block itself -- lane j keeps column j of the 32 x 32 diagonal block in registers
// and the 32 unknowns go by, last first: x_i = y_i / L_ii in lane i, broadcast by v_readlane, y_j -= L_ij x_i in the lanes j < i --;
// the other wavefronts then take the block's unknowns out of everything above: thread t keeps column t of the block row L[blk, 0:k0]
// in registers.  Nothing that is loaded depends on x: both register sets are requested one block ahead.  yv holds y on entry and x on
// return; rd_all = 1 / L_ii of all n unknowns (kept from the factorisation); needs n - 32 <= blockDim - 64.
__device__ __forceinline__ void chol_backward_blocks(const BADev &D, double *yv, const double *rd_all, double *s_x)
{
    const int n = D.nf, ld = D.nfp, tid = threadIdx.x, lane = tid & 63, t = tid - 64;
    const bool w0 = tid < 64;
    const double *S = D.S;
    const int nblk = (n + CH_NB - 1) / CH_NB;
    double cur[CH_NB], nxt[CH_NB], nx2[CH_NB];                   // two blocks ahead: a block's own work is ~1 us, its 32 loads per thread ~3 us
    auto load = [&](int k0, int nb, double (&v)[CH_NB]) {
        const double *col = S + (long long)k0 * ld + (w0 ? k0 + lane : t);
        const bool mine = w0 ? lane < nb : t < k0;
#pragma unroll
        for (int i = 0; i < CH_NB; i++) v[i] = (mine && i < nb && (!w0 || i > lane)) ? col[(long long)i * ld] : 0.0;   // w0: L[i][lane] of the diagonal block; else L[k0 + i][t]
    };
    load((nblk - 1) * CH_NB, n - (nblk - 1) * CH_NB, cur);
#pragma unroll
    for (int i = 0; i < CH_NB; i++) nxt[i] = 0.0;
    if (nblk > 1) load((nblk - 2) * CH_NB, CH_NB, nxt);
    for (int blk = nblk - 1; blk >= 0; blk--) {
        const int k0 = blk * CH_NB, nb = min(CH_NB, n - k0);
#pragma unroll
        for (int i = 0; i < CH_NB; i++) nx2[i] = 0.0;
        if (blk > 1) load(k0 - 2 * CH_NB, CH_NB, nx2);
        __syncthreads();                                         // y carries every later block's update
        if (w0) {
            double y = lane < nb ? yv[k0 + lane] : 0.0;
            const double rd = lane < nb ? rd_all[k0 + lane] : 0.0;
            int ln = lane;
            asm volatile("" : "+v"(ln));                             // (keeps the 64 lane masks below out of spilled scalar registers)
#pragma unroll
            for (int i = CH_NB - 1; i >= 0; i--) {
                const double xl = y * rd;
                const double xi = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(xl), i), __builtin_amdgcn_readlane(__double2loint(xl), i));
                y = ln == i ? xi : (ln < i ? y - cur[i] * xi : y);
            }
            if (lane < CH_NB) s_x[lane] = y;
            if (lane < nb) yv[k0 + lane] = y;
        }
        __syncthreads();
        if (!w0 && t < k0) {
            double acc = yv[t];
#pragma unroll
            for (int i = 0; i < CH_NB; i++) acc -= cur[i] * s_x[i];
            yv[t] = acc;
        }
#pragma unroll
        for (int i = 0; i < CH_NB; i++) { cur[i] = nxt[i]; nxt[i] = nx2[i]; }
    }
    __syncthreads();
}

__device__ __forceinline__ void b_ba_cholesky(const BADev &D)
{
    BACtl *ctl = D.ctl;
    if (ctl->done) return;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    double *L11 = (double *)smem_raw;                       // CH_NB x CH_LDP : diagonal block / its inverse
    double *yv = L11 + CH_NB * CH_LDP;                      // nfp
    double *P = yv + D.nfp;                                 // (n - CH_NB) x CH_LDP : panel below the diagonal block
    double *rd_all = P + (size_t)((max(0, D.nf - CH_NB) + 15) & ~15) * CH_LDP;   // nfp: reciprocal pivots of all unknowns (backward substitution)
    const int n = D.nf, ld = D.nfp, tid = threadIdx.x, nt = blockDim.x;
    const int wave = tid >> 6, lane = tid & 63;
    __shared__ int s_fail;
    __shared__ double s_red[32][33];
    __shared__ double s_rdiag[CH_NB];                        // 1 / L11[j][j] of the current diagonal block
    __shared__ double s_yk[CH_NB];                           // the block's part of the forward solution (the right-hand side as a panel row)
    double *S = D.S;
    // The right-hand side rides through the factorisation as one more row of the panel: solving its block against L11 IS the
    // forward substitution of that block, and its trailing update (rhs_rest -= P y_blk) replaces the forward pass of the
    // triangular solves (ten blocks of partial sums over L in L2, three barriers each).  Needs a free panel thread.
    const bool rhs_row = n - CH_NB + 1 <= nt - 128;
    // (S was assembled by k_ba_assemble: in here, one workgroup walking the n^2 entries took 85 us of latency)
    for (int i = tid; i < D.nfp; i += nt) yv[i] = i < n ? D.scale_f[i] * (D.bf[i] - D.v[i]) : 0.0;
    if (tid == 0) s_fail = 0;
    __syncthreads();

    unsigned long long tk[6] = {0, 0, 0, 0, 0, 0}, tc = wall_clock64();
#define CH_TICK(i) do { const unsigned long long t_ = wall_clock64(); tk[i] += t_ - tc; tc = t_; } while (0)
    for (int k0 = 0; k0 < n; k0 += CH_NB) {
        const int nb = min(CH_NB, n - k0);
        const int m = n - k0 - nb;                          // rows below the diagonal block
        // (a) diagonal block -> LDS (identity padding when nb < 32), panel rows -> LDS (coalesced)
        for (int e = tid; e < CH_NB * CH_NB; e += nt) {
            const int i = e >> 5, j = e & 31;
            double v = (i == j) ? 1.0 : 0.0;
            if (i < nb && j <= i) v = S[(long long)(k0 + i) * ld + k0 + j];
            L11[i * CH_LDP + j] = v;
        }
        // (eight loads in flight per thread: a load -> LDS store loop pays one L2 round trip per element)
        for (int e0 = tid; e0 < m * CH_NB; e0 += 8 * nt) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int e = e0 + u * nt, t = e >> 5, j = e & 31;
                v[u] = (e < m * CH_NB && j < nb) ? S[(long long)(k0 + nb + t) * ld + k0 + j] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int e = e0 + u * nt;
                if (e < m * CH_NB) P[(e >> 5) * CH_LDP + (e & 31)] = v[u];
            }
        }
        __syncthreads();
        CH_TICK(0);
        // (b) + (c), pipelined through LDS.  Wavefront 0 factors the diagonal block (left-looking, lane i owns row i in
        //     registers, one LDS sync per column) and PUBLISHES its columns in groups of four (L11[.][c], the reciprocal pivots,
        //     then a work-group barrier; a per-column flag with spinning consumers made the register allocator spill the row
        //     arrays).  The other wavefronts solve the panel X L11^T = A21 one row per thread and trail the
        //     factorisation by one column instead of waiting for all 32: the panel solve (9 us per panel as a phase of its own)
        //     hides behind the 5 us pivot chain.
        if (wave == 0) {
            double a[CH_NB];
#pragma unroll
            for (int j = 0; j < CH_NB; j++) a[j] = lane < CH_NB ? L11[lane * CH_LDP + j] : 0.0;
            bool fail = false;
            // (the lane index of THIS panel step: compared against the 32 column numbers below.  Without the laundering the compiler
            // hoists all 64 lane masks out of the panel loop and parks them in spilled scalar registers -- 470 v_writelane / 1000
            // v_readlane with their wait states, on the one wavefront everybody waits for)
            int ln = lane;
            asm volatile("" : "+v"(ln));
            // Column c needs  a[c] - sum_{k<c} a[k] L[c][k]  of every row.  Round 4: the terms of the columns published two
            // barriers ago and earlier (k < 4 (c/4 - 1)) are taken out of the future columns by the HELPER wavefront below, in LDS,
            // while this wavefront works on the current group of four -- it had 90 instructions per column at c = 20, two thirds of
            // them those terms, and every other wavefront of the kernel waits for it.  What stays here: the 4 .. 7 terms of the last
            // two groups (this wavefront's own registers), the same order k = 0, 1, .. as ever (bit-identical factor).  All of them
            // but the last (k = c-1) are known one column earlier and are accumulated while the previous pivot's rsqrt chain is in
            // flight -- except for the first column of a group, whose LDS value is final only after the barrier just passed.
            double pnext = a[0];
#pragma unroll
            for (int c = 0; c < CH_NB; c++) {
                double sacc;
                if ((c & (CH_GRP - 1)) == 0 && c >= 2 * CH_GRP) {
#pragma unroll
                    for (int q = 0; q < CH_GRP; q++) a[c + q] = ln < CH_NB ? L11[ln * CH_LDP + c + q] : 0.0;   // with the helper's terms
                    sacc = a[c];
#pragma unroll
                    for (int k = c - CH_GRP; k < c; k++) sacc -= a[k] * L11[c * CH_LDP + k];
                } else {
                    sacc = pnext;
                    if (c > 0) sacc -= a[c - 1] * L11[c * CH_LDP + c - 1];          // row c of L, final for k < c (broadcast read)
                }
                const double d = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(sacc), c), __builtin_amdgcn_readlane(__double2loint(sacc), c));
                if (c + 1 < CH_NB && !(((c + 1) & (CH_GRP - 1)) == 0 && c + 1 >= 2 * CH_GRP)) {
                    const int kmin = (c + 1) / CH_GRP >= 1 ? CH_GRP * ((c + 1) / CH_GRP - 1) : 0;
                    pnext = a[c + 1];
#pragma unroll
                    for (int k = kmin; k < c; k++) pnext -= a[k] * L11[(c + 1) * CH_LDP + k];
                }
                if (!(d > 0.0) || !isfinite(d)) fail = true;
                // pivot through 1/sqrt(d): v_rsq_f64 seed (~2^-26) + two Newton steps, then L[c][c] = d r with one Heron
                // correction and L[i][c] = sacc r -- 9 dependent instructions instead of the ~25 of sqrt() followed by a
                // division, 32 times per block on the kernel's longest serial chain (and 15 KB less unrolled code)
                double r = __builtin_amdgcn_rsq(d);
                r = fma(0.5 * r, fma(-(d * r), r, 1.0), r);
                r = fma(0.5 * r, fma(-(d * r), r, 1.0), r);
                double dj = d * r;
                dj = fma(0.5 * r, fma(-dj, dj, d), dj);
                const double l = ln == c ? dj : sacc * r;
                a[c] = ln >= c ? l : 0.0;
                if (ln < CH_NB) L11[ln * CH_LDP + c] = a[c];                 // (lanes < c write the 0 of the upper triangle: never read)
                // reciprocal pivot 1 / L[c][c]: r refined by one Newton step of the reciprocal (two FMAs, no division)
                if (ln == c) { const double rc = fma(r, fma(-dj, r, 1.0), r); s_rdiag[c] = rc; rd_all[k0 + c] = rc; }
                wave_lds_sync();
                if ((c & (CH_GRP - 1)) == CH_GRP - 1) __syncthreads();   // columns c-CH_GRP+1 .. c are published: the panel wavefronts may use them
            }
            if (fail && lane == 0) s_fail = 1;
        } else if (wave == 4) {
            // the helper (same SIMD as wavefront 0, no panel rows): before barrier g the columns of the groups < g are published; it
            // takes the terms of group g-1 out of the columns of the groups > g (row per lane, two columns at a time), in place
            const int hi = lane & 31, hh = lane >> 5;
#pragma unroll
            for (int g = 0; g < CH_NB / CH_GRP; g++) {
                if (g >= 1) {
                    const int kb = CH_GRP * (g - 1);
                    double lk4[CH_GRP];
#pragma unroll
                    for (int q = 0; q < CH_GRP; q++) lk4[q] = L11[hi * CH_LDP + kb + q];
#pragma unroll
                    for (int jj = CH_GRP * (g + 1); jj < CH_NB; jj += 2) {
                        const int j = jj + hh;
                        double acc = L11[hi * CH_LDP + j];
#pragma unroll
                        for (int q = 0; q < CH_GRP; q++) acc -= lk4[q] * L11[j * CH_LDP + kb + q];
                        L11[hi * CH_LDP + j] = acc;
                    }
                }
                __syncthreads();
            }
        } else {
            // left-looking per row (x[32] in registers, row j of L read as one contiguous LDS row).  Every panel wavefront
            // passes the same 8 work-group barriers as wavefront 0, whether its threads own a row or not.
            // (wavefronts 1-3 and 5-7 take rows 0 .. 383; two rows per thread on three wavefronts would halve the broadcast reads of
            // L11 -- 1 KB comes back per ds_read_b128 whatever the number of rows it serves -- but x and z together need more
            // than the 256 registers the kernel has: measured with spills, 202 us against 89)
            const int t = wave < 4 ? tid - 64 : tid - 128;
            const bool has = t < m;
            const bool rhs = rhs_row && t == m;                 // the thread after the last panel row takes the right-hand side
            double x[CH_NB];
#pragma unroll
            for (int j = 0; j < CH_NB; j++) x[j] = has ? P[t * CH_LDP + j] : (rhs ? yv[k0 + j] : 0.0);
#pragma unroll
            for (int j = 0; j < CH_NB; j++) {
                if ((j & (CH_GRP - 1)) == 0) {
                    // x[j-1] must be finished BEFORE the barrier: without this artificial use the scheduler drains all eight
                    // barriers first -- loading the whole block into registers (992 VGPRs: spills) -- and computes afterwards,
                    // which also serialises the panel solve behind the factorisation again
                    if (j > 0) asm volatile("" ::"v"(x[j - 1]) : "memory");
                    __syncthreads();                           // columns j .. j+3 of L11 and their reciprocal pivots are there
                }
                double acc = x[j];
#pragma unroll
                for (int k = 0; k < j; k++) acc -= x[k] * L11[j * CH_LDP + k];
                x[j] = acc * s_rdiag[j];
            }
            if (has) {
#pragma unroll
                for (int j = 0; j < CH_NB; j++) P[t * CH_LDP + j] = x[j];
            }
            if (rhs) {
#pragma unroll
                for (int j = 0; j < CH_NB; j++) { s_yk[j] = x[j]; if (j < nb) yv[k0 + j] = x[j]; }
            }
        }
        __syncthreads();
        // rows beyond the pipelined ones (only for reduced systems of more than ~480 unknowns): plain pass on the LDS rows, the
        // block is complete.  Rolled on purpose: an unrolled copy of the 496-term row solve is 12 KB of code, and this kernel has
        // to stay inside the 64 KB instruction cache (round 4: at 77 KB every panel step re-fetched its code from L2).
        for (int t = tid + 384; t < m; t += nt) {
            double *xr = P + t * CH_LDP;
#pragma nounroll
            for (int j = 0; j < CH_NB; j++) {
                double acc = xr[j];
#pragma nounroll
                for (int k = 0; k < j; k++) acc -= xr[k] * L11[j * CH_LDP + k];
                xr[j] = acc * s_rdiag[j];
            }
        }
        __syncthreads();
        if (rhs_row) {
            // trailing update of the right-hand side: rhs[below] -= P y_blk
            for (int i = tid; i < m; i += nt) {
                double acc = yv[k0 + nb + i];
#pragma unroll
                for (int j = 0; j < CH_NB; j++) acc -= P[i * CH_LDP + j] * s_yk[j];
                yv[k0 + nb + i] = acc;
            }
        }
        CH_TICK(1);
        if (s_fail) break;
        // factored block and panel back to HBM (coalesced)
        for (int e = tid; e < nb * nb; e += nt) {
            const int i = e / nb, j = e - i * nb;
            if (j <= i) S[(long long)(k0 + i) * ld + k0 + j] = L11[i * CH_LDP + j];
        }
        for (int e = tid; e < m * CH_NB; e += nt) {
            const int t = e >> 5, j = e & 31;
            if (j < nb) S[(long long)(k0 + nb + t) * ld + k0 + j] = P[t * CH_LDP + j];
        }
        CH_TICK(2);
        // (d) trailing update  A22 -= P P^T  (lower triangle) on the fp64 matrix cores: one wavefront per 16x16 tile,
        //     8 x v_mfma_f64_16x16x4_f64 over the 32 panel columns.  Operand layout (cdna_hip_programming.md, f64 MFMA):
        //     A: lane holds A[lane & 15][lane >> 4], B: lane holds B[lane >> 4][lane & 15] -- both are rows of the LDS
        //     panel --, C/D: col = lane & 15, row = (lane >> 4) + 4 * reg.  S stays in HBM/L2; a tile is read, updated
        //     and written once per panel step.
        {
            typedef double d4 __attribute__((ext_vector_type(4)));
            const int mb = (m + 15) >> 4, nwv = nt >> 6;
            const int lr = lane & 15, lk = lane >> 4;
            // A wavefront takes the tiles wv, wv + nwv, .. of the row-major lower-triangle enumeration, two at a time (two
            // independent MFMA chains).  Round 4: the phase was a SUM of its parts (knock-outs: 24 us of tile bookkeeping -- a
            // double-precision sqrt per tile index, 64-bit multiplies per element address, four predicates per element --, 31 us of
            // MFMA, 9 us of loads, 6 us of LDS reads, 4 us of stores; two wavefronts per SIMD overlap little).  Now the tile
            // walk is integer arithmetic on the scalar unit (wave-uniform), an element's address is a uniform base + one of four
            // per-lane constants, operand rows are read unpredicated (garbage rows >= m only reach rows / columns that are not
            // stored), and the old values of the next pair are requested before the chains of the current pair run.
            const int ntile = mb * (mb + 1) / 2;
            const int wv = __builtin_amdgcn_readfirstlane(wave);
            auto advance = [&](int &bi, int &bj, int step) { bj += step; while (bj > bi) { bj -= bi + 1; bi++; } };
            int lo[4];                                              // element (lk + 4 r, lr) of a tile, in doubles from the tile's corner
#pragma unroll
            for (int r = 0; r < 4; r++) lo[r] = (lk + 4 * r) * ld + lr;
            double *Sc = S + (long long)(k0 + nb) * ld + k0 + nb;      // corner of the trailing matrix
            const double *Pl = P + lr * CH_LDP + lk;                   // this lane's operand element of tile row 0
            auto corner = [&](int bi, int bj) { return Sc + ((long long)bi * ld + bj) * 16; };
            auto okmask = [&](int bi, int bj, int r) { return (16 * bi + lk + 4 * r < m) && (bi != bj || lr <= lk + 4 * r); };
            auto fetch = [&](int bi, int bj, bool has, double (&o)[4]) {
                const double *c = corner(bi, bj);
#pragma unroll
                for (int r = 0; r < 4; r++) o[r] = (has && okmask(bi, bj, r)) ? c[lo[r]] : 0.0;
            };
            int bi0 = 0, bj0 = 0, bi1, bj1;
            advance(bi0, bj0, wv);
            bi1 = bi0; bj1 = bj0; advance(bi1, bj1, nwv);
            double old0[4], old1[4];
            fetch(bi0, bj0, wv < ntile, old0);
            fetch(bi1, bj1, wv + nwv < ntile, old1);
            for (int t0 = wv; t0 < ntile; t0 += 2 * nwv) {
                const bool has1 = t0 + nwv < ntile;
                int nbi0 = bi1, nbj0 = bj1, nbi1, nbj1;
                advance(nbi0, nbj0, nwv);
                nbi1 = nbi0; nbj1 = nbj0; advance(nbi1, nbj1, nwv);
                double nold0[4], nold1[4];
                fetch(nbi0, nbj0, t0 + 2 * nwv < ntile, nold0);
                fetch(nbi1, nbj1, t0 + 3 * nwv < ntile, nold1);
                const double *pa0 = Pl + bi0 * (16 * CH_LDP), *pb0 = Pl + bj0 * (16 * CH_LDP);
                const double *pa1 = Pl + (has1 ? bi1 : bi0) * (16 * CH_LDP), *pb1 = Pl + (has1 ? bj1 : bj0) * (16 * CH_LDP);
                d4 c0 = {0., 0., 0., 0.}, c1 = {0., 0., 0., 0.};
#pragma unroll
                for (int kk = 0; kk < CH_NB / 4; kk++) {
                    c0 = __builtin_amdgcn_mfma_f64_16x16x4f64(pa0[4 * kk], pb0[4 * kk], c0, 0, 0, 0);
                    c1 = __builtin_amdgcn_mfma_f64_16x16x4f64(pa1[4 * kk], pb1[4 * kk], c1, 0, 0, 0);
                }
                double *q0 = corner(bi0, bj0), *q1 = corner(bi1, bj1);
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    if (okmask(bi0, bj0, r)) q0[lo[r]] = old0[r] - c0[r];
                    if (has1 && okmask(bi1, bj1, r)) q1[lo[r]] = old1[r] - c1[r];
                }
                bi0 = nbi0; bj0 = nbj0; bi1 = nbi1; bj1 = nbj1;
#pragma unroll
                for (int r = 0; r < 4; r++) { old0[r] = nold0[r]; old1[r] = nold1[r]; }
            }
        }
        __syncthreads();
        CH_TICK(3);
    }
    if (s_fail) { if (tid == 0) ctl->lin_fail = 1; return; }

    CH_TICK(4);
    // forward substitution rode along as a panel row (rhs_row: the host sends systems of more than 479 unknowns to the HBM path);
    // backward substitution from the factor itself -- no inverse diagonal blocks (rounds 1-3 computed them here: 20 us and 12 KB of
    // unrolled code in a kernel that has to fit the instruction cache)
    chol_backward_blocks(D, yv, rd_all, &s_red[0][0]);

    for (int i = tid; i < n; i += nt) D.yf[i] = yv[i];
    CH_TICK(5);
    if (tid == 0) for (int i = 0; i < 6; i++) ctl->dbg[i] = tk[i];
#undef CH_TICK
}
__global__ __launch_bounds__(512) void k_ba_cholesky(BADev D) { b_ba_cholesky(D); }
__global__ __launch_bounds__(512) void k_ba_cholesky_B(const BADev *__restrict__ arr) { const BADev &D = arr[blockIdx.z]; b_ba_cholesky(D); }

// Blocked right-looking Cholesky of the reduced system on HBM, three kernels per 32-column panel:
//   k_chol_diag  (1 wavefront): factor the diagonal block in LDS (same register-row algorithm as k_ba_cholesky), write it back, and
//                its inverse (for the triangular solves) to Linv
//   k_chol_panel (64 rows per work-group): X L11^T = A21 by substitution, one row per thread
//   k_chol_trail (one 32 x 32 tile per work-group, lower triangle): A22 -= X X^T
// then k_chol_solve (1 work-group): the two triangular solves.  ~3 * nf / 32 launches per LM iteration: this path is for the
// loop-closure / offline BAs (hundreds of keyframes), where a solve takes milliseconds either way.
__global__ __launch_bounds__(64) void k_chol_diag(BADev D, int k0)
{
    BACtl *ctl = D.ctl;
    if (ctl->done || ctl->lin_fail) return;
    __shared__ double L11[CH_NB * CH_LDP];
    const int n = D.nf, ld = D.nfp, lane = threadIdx.x;
    const int nb = min(CH_NB, n - k0);
    double *S = D.S;
    for (int e = lane; e < CH_NB * CH_NB; e += 64) {
        const int i = e >> 5, j = e & 31;
        double v = (i == j) ? 1.0 : 0.0;
        if (i < nb && j <= i) v = S[(long long)(k0 + i) * ld + k0 + j];
        L11[i * CH_LDP + j] = v;
    }
    wave_lds_sync();
    double a[CH_NB];
#pragma unroll
    for (int j = 0; j < CH_NB; j++) a[j] = lane < CH_NB ? L11[lane * CH_LDP + j] : 0.0;
    bool fail = false;
    double pnext = a[0];
#pragma unroll
    for (int c = 0; c < CH_NB; c++) {
        double sacc = pnext;
        if (c > 0) sacc -= a[c - 1] * L11[c * CH_LDP + c - 1];
        const double d = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(sacc), c), __builtin_amdgcn_readlane(__double2loint(sacc), c));
        if (c + 1 < CH_NB) {
            pnext = a[c + 1];
#pragma unroll
            for (int k = 0; k < c; k++) pnext -= a[k] * L11[(c + 1) * CH_LDP + k];
        }
        if (!(d > 0.0) || !isfinite(d)) fail = true;
        double r = __builtin_amdgcn_rsq(d);
        r = fma(0.5 * r, fma(-(d * r), r, 1.0), r);
        r = fma(0.5 * r, fma(-(d * r), r, 1.0), r);
        double dj = d * r;
        dj = fma(0.5 * r, fma(-dj, dj, d), dj);
        const double l = lane == c ? dj : sacc * r;
        a[c] = lane >= c ? l : 0.0;
        if (lane >= c && lane < CH_NB) L11[lane * CH_LDP + c] = a[c];
        if (lane == c) L11[c * CH_LDP + CH_NB] = fma(r, fma(-dj, r, 1.0), r);          // reciprocal pivot in the padding column
        wave_lds_sync();
    }
    if (__builtin_amdgcn_ballot_w64(fail) != 0) { if (lane == 0) ctl->lin_fail = 1; return; }
    for (int e = lane; e < nb * nb; e += 64) {
        const int i = e / nb, j = e - i * nb;
        if (j <= i) S[(long long)(k0 + i) * ld + k0 + j] = L11[i * CH_LDP + j];
    }
    if (lane < CH_NB) {                                                 // inverse block: lane j solves L x = e_j
        double x[CH_NB];
#pragma unroll
        for (int i = 0; i < CH_NB; i++) {
            double acc = (i == lane) ? 1.0 : 0.0;
#pragma unroll
            for (int k = 0; k < i; k++) acc -= L11[i * CH_LDP + k] * x[k];
            x[i] = i < lane ? 0.0 : acc * L11[i * CH_LDP + CH_NB];
        }
        double *dst = D.Linv + (long long)(k0 / CH_NB) * CH_NB * CH_NB;
#pragma unroll
        for (int i = 0; i < CH_NB; i++) dst[i * CH_NB + lane] = x[i];
    }
}

__global__ __launch_bounds__(64) void k_chol_panel(BADev D, int k0)
{
    const BACtl *ctl = D.ctl;
    if (ctl->done || ctl->lin_fail) return;
    __shared__ double L11[CH_NB * CH_LDP];
    __shared__ double X[64 * CH_LDP];                                   // the work-group's 64 panel rows (a thread's row stays in LDS: the fully
                                                                        // unrolled register version made the scheduler hoist all 496 loads of L11
                                                                        // -- 512 VGPRs, 624 spills -- and miscomputed from column 12 on)
    const int n = D.nf, ld = D.nfp, lane = threadIdx.x;
    const int nb = min(CH_NB, n - k0), m = n - k0 - nb;
    double *S = D.S;
    for (int e = lane; e < CH_NB * CH_NB; e += 64) {
        const int i = e >> 5, j = e & 31;
        double v = (i == j) ? 1.0 : 0.0;
        if (i < nb && j <= i) v = S[(long long)(k0 + i) * ld + k0 + j];
        L11[i * CH_LDP + j] = v;
    }
    const int t0 = blockIdx.x * 64;
    for (int e = lane; e < 64 * CH_NB; e += 64) {                       // coalesced: 32 consecutive columns of one row per half wavefront
        const int r = e >> 5, j = e & 31;
        X[r * CH_LDP + j] = (t0 + r < m && j < nb) ? S[(long long)(k0 + nb + t0 + r) * ld + k0 + j] : 0.0;
    }
    __syncthreads();
    double *x = X + lane * CH_LDP;
    for (int j = 0; j < CH_NB; j++) {
        double acc = x[j];
        const double *lr = L11 + j * CH_LDP;
        for (int k = 0; k < j; k++) acc -= x[k] * lr[k];
        x[j] = acc / lr[j];
    }
    __syncthreads();
    for (int e = lane; e < 64 * CH_NB; e += 64) {
        const int r = e >> 5, j = e & 31;
        if (t0 + r < m && j < nb) S[(long long)(k0 + nb + t0 + r) * ld + k0 + j] = X[r * CH_LDP + j];
    }
}

__global__ __launch_bounds__(256) void k_chol_trail(BADev D, int k0)
{
    const BACtl *ctl = D.ctl;
    if (ctl->done || ctl->lin_fail) return;
    __shared__ double A[32][33], B[32][33];
    const int n = D.nf, ld = D.nfp, tid = threadIdx.x;
    const int nb = min(CH_NB, n - k0), m = n - k0 - nb;
    // lower-triangular tile index -> (bi, bj), bj <= bi
    int t = blockIdx.x, bi = 0;
    while (t > bi) { t -= bi + 1; bi++; }
    const int bj = t;
    double *S = D.S;
    for (int e = tid; e < 32 * 32; e += 256) {
        const int r = e >> 5, c = e & 31;
        const int ia = bi * 32 + r, ib = bj * 32 + r;
        A[r][c] = (ia < m && c < nb) ? S[(long long)(k0 + nb + ia) * ld + k0 + c] : 0.0;
        B[r][c] = (ib < m && c < nb) ? S[(long long)(k0 + nb + ib) * ld + k0 + c] : 0.0;
    }
    __syncthreads();
    const int r0 = (tid >> 4) * 2, c0 = (tid & 15) * 2;                 // 2 x 2 outputs per thread
    double acc[2][2] = {{0, 0}, {0, 0}};
    for (int k = 0; k < 32; k++) {
        const double a0 = A[r0][k], a1 = A[r0 + 1][k], b0 = B[c0][k], b1 = B[c0 + 1][k];
        acc[0][0] += a0 * b0; acc[0][1] += a0 * b1; acc[1][0] += a1 * b0; acc[1][1] += a1 * b1;
    }
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 2; j++) {
            const int gi = bi * 32 + r0 + i, gj = bj * 32 + c0 + j;
            if (gi < m && gj <= gi) S[(long long)(k0 + nb + gi) * ld + k0 + nb + gj] -= acc[i][j];
        }
}

__global__ __launch_bounds__(512) void k_chol_solve(BADev D)
{
    const BACtl *ctl = D.ctl;
    if (ctl->done || ctl->lin_fail) return;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    double *L11 = (double *)smem_raw;                       // CH_NB x CH_LDP
    double *yv = L11 + CH_NB * CH_LDP;                      // nfp
    __shared__ double s_red[32][33];
    const int n = D.nf, tid = threadIdx.x, nt = blockDim.x;
    for (int i = tid; i < D.nfp; i += nt) yv[i] = i < n ? D.scale_f[i] * (D.bf[i] - D.v[i]) : 0.0;
    __syncthreads();
    chol_trisolve(D, L11, yv, s_red);
    for (int i = tid; i < n; i += nt) D.yf[i] = yv[i];
}

