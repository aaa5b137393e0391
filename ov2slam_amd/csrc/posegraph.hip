// posegraph.hip -- Optimizer::localPoseGraph / fullPoseGraph for gfx950 (src/optimizer.cpp:2346-2591, :2783-2865 of the reference).
//
// SE(3) poses tied by LeftSE3RelativePoseError blocks (src/ceres_parametrization.cpp:30-102), no loss function,
// SPARSE_NORMAL_CHOLESKY / LM.  An edge couples two variable poses only when they are neighbours among the variable poses, so
// J^T J + D^2 is block-tridiagonal with 6x6 blocks and falls into independent segments; the exact solve is a block Cholesky
// recurrence along each segment.
//
// Design: ONE launch, one 256-thread work-group per problem (grid.x = item), the control block in LDS, thread 0 calls the shared
// trust-region rules (ba_core.hpp) between two barriers.  Per LM iteration:
//   linearise   a lane per edge: log, the two adjoints, the two 6x6 products; r and the un-scaled J0, J1 go to HBM
//   assemble    a lane per (variable pose, column): the column of the diagonal block, of the coupling to the next variable pose
//               and of J^T r, summed over the pose's incident edges in the CALLER's edge order (a host-staged table) -- no
//               floating-point atomics, the same bytes on every run
//   solve       segments shorter than PG_CR_MIN side by side, a lane per segment: block Cholesky recurrence along the chain;
//               longer ones (localPoseGraph: ONE segment of up to a thousand poses) by the whole work-group: block cyclic
//               reduction, ceil(log2 n) levels of independent 6x6 eliminations instead of n dependent steps
//   candidate   a lane per pose (Exp(delta) T), a lane per edge (cost), fixed-order work-group sums
// 256 threads: the segment lane holds three 6x6 blocks in registers and must not spill.
#include "common.hpp"
#include <cmath>

#pragma clang fp contract(off)
#include "ba_core.hpp"            // (after the pragma: the shared functions are compiled without contraction here)
#include "se3_dev.hpp"            // PgSE3, pg_load, pg_mul, pg_inv, pg_log, pg_exp: shared with motion.hip

#define PG_THREADS 256
// Segments of at least this many poses take the cyclic-reduction path.  One segment, whole solves on an MI355X:
// 17 poses 1.06 ms by the recurrence / 1.10 ms by cyclic reduction, 64 poses 3.1 / 1.3 ms, 257 poses 17.6 / 3.0 ms, 1500 poses
// 86 / 10.5 ms.  Long segments are reduced one after the other while the short ones run side by side, a lane each (fullPoseGraph:
// hundreds of segments of 5-20 poses, 0.5 ms by the recurrence / 6 ms through the reduction), hence a constant above the break-even.
#define PG_CR_MIN 32

struct PgOut { int iterations, num_successful_steps, termination, n_trace; double initial_cost, final_cost; };

// byte offsets into the call's arena
struct PgItem {
    int n_poses, n_var, n_act, n_seg;
    long long o_x, o_vidx, o_ei, o_ej, o_eT, o_esi, o_incp, o_inc, o_seg;     // staged by the host (o_x: in / out)
    long long o_cand, o_r, o_J, o_H, o_C, o_g, o_b, o_scale, o_y, o_L, o_W, o_G, o_K;   // workspace
};

struct PgArgs {
    uint8_t *arena;
    const PgItem *items;
    PgOut *out;
    BAOpt O; double initial_radius;
    BAIterRec *trace;             // the single-problem solve with OV2_OPT_BA_TRACE, else NULL
};

// ---------------------------------------------------------------------------------- SE(3), as Sophus::SE3d computes it: se3_dev.hpp
// T' = Exp(delta) * T   (se3left_parametrization.hpp:41-60)
__device__ __forceinline__ void pg_se3_left_plus(const double *pose, const double *a, double *out)
{
    const PgSE3 R = pg_mul(pg_exp(a), pg_load(pose));
    pg_store(R, out);
}

// si * (A | B ; 0 | A) * Adj(T) -> J (6x6 row-major), A = I + sg W / 2, B = sg P / 2 (W = hat(omega), P = hat(rho)), times `lead`
__device__ __forceinline__ void pg_jac_block(double sg, double lead, const double *v, const PgSE3 &T, double *J)
{
    double R[9], S[9], A[9], B[9];
    d_quat_to_R(T.q, R);
    const double Ht[9] = {0, -T.t[2], T.t[1], T.t[2], 0, -T.t[0], -T.t[1], T.t[0], 0};
    const double W[9] = {0, -v[5], v[4], v[5], 0, -v[3], -v[4], v[3], 0};
    const double P[9] = {0, -v[2], v[1], v[2], 0, -v[0], -v[1], v[0], 0};
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            S[3 * i + j] = Ht[3 * i] * R[j] + Ht[3 * i + 1] * R[3 + j] + Ht[3 * i + 2] * R[6 + j];        // hat(t) R
            A[3 * i + j] = (i == j ? 1.0 : 0.0) + 0.5 * (sg * W[3 * i + j]);
            B[3 * i + j] = 0.5 * (sg * P[3 * i + j]);
        }
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double ar = A[3 * i] * R[j] + A[3 * i + 1] * R[3 + j] + A[3 * i + 2] * R[6 + j];
            const double as = A[3 * i] * S[j] + A[3 * i + 1] * S[3 + j] + A[3 * i + 2] * S[6 + j];
            const double br = B[3 * i] * R[j] + B[3 * i + 1] * R[3 + j] + B[3 * i + 2] * R[6 + j];
            J[6 * i + j] = lead * ar;
            J[6 * i + 3 + j] = lead * (as + br);
            J[6 * (i + 3) + j] = 0.0;
            J[6 * (i + 3) + 3 + j] = lead * ar;
        }
}

// one LeftSE3RelativePoseError::Evaluate: r (6), and with JAC the local Jacobians J0, J1 (6x6 row-major, first six columns)
template <bool JAC>
__device__ __forceinline__ void pg_edge(const double *Pi, const double *Pj, const double *Tm, double si, double *r, double *J0, double *J1)
{
    const PgSE3 T0 = pg_load(Pi), T1 = pg_load(Pj), M = pg_load(Tm);
    const PgSE3 Tc1w = pg_inv(T1);
    const PgSE3 err = pg_mul(pg_mul(Tc1w, T0), M);
    double v[6];
    pg_log(err, v);
#pragma unroll
    for (int k = 0; k < 6; k++) r[k] = si * v[k];
    if (JAC) {
        pg_jac_block(-1.0, si, v, Tc1w, J0);                             //  sqrt_info (I - J_c / 2) Adj(Twc1^-1)
        pg_jac_block(1.0, -si, v, pg_inv(pg_mul(T0, M)), J1);            // -sqrt_info (I + J_c / 2) Adj((Twc0 Tc0c1)^-1)
    }
}

// ---------------------------------------------------------------------------------- the work-group's pieces
// deterministic work-group maximum, result in every thread
__device__ __forceinline__ double pg_block_max(double v, double *sh)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    double t = 0;
    for (int w = 0; w < nw; w++) t = fmax(t, sh[w]);
    return t;
}

struct PgDev {
    int n_poses, n_var, n_act, n_seg;
    double *x, *cand;
    const int *vidx, *ei, *ej, *incp, *inc, *seg, *vpose;      // seg: (first, end) per segment; vpose: pose of a variable
    const double *eT, *esi;
    double *r, *J, *H, *C, *g, *b, *scale, *y, *L, *W, *G, *K;
};

// cost of the edges at `poses` (thread-local partial); JAC: also r and the un-scaled Jacobians
template <bool JAC>
__device__ __forceinline__ double pg_evaluate(const PgDev &D, const double *poses)
{
    double cost = 0;
    for (int e = threadIdx.x; e < D.n_act; e += blockDim.x) {
        double r[6], J0[36], J1[36];
        pg_edge<JAC>(poses + 7 * D.ei[e], poses + 7 * D.ej[e], D.eT + 7 * (size_t)e, D.esi[e], r, J0, J1);
        double sq = 0;
#pragma unroll
        for (int k = 0; k < 6; k++) sq += r[k] * r[k];
        cost += 0.5 * sq;
        if (JAC) {
            double *ro = D.r + 6 * (size_t)e, *Jo = D.J + 72 * (size_t)e;
#pragma unroll
            for (int k = 0; k < 6; k++) ro[k] = r[k];
#pragma unroll
            for (int k = 0; k < 36; k++) { Jo[k] = J0[k]; Jo[36 + k] = J1[k]; }
        }
    }
    return cost;
}

// column c of variable pose k: H_kk[:, c], C_k[:, c] (coupling of k's columns to column c of pose k + 1), b = Js^T r, g = J^T r;
// Js = J scale, summed over the incident (edge, side) entries in the caller's edge order
__device__ __forceinline__ void pg_assemble(const PgDev &D)
{
    for (int t = threadIdx.x; t < 6 * D.n_var; t += blockDim.x) {
        const int k = t / 6, c = t - 6 * k;
        const double sc = D.scale[t];
        const double *sk = D.scale + 6 * k;
        double h[6] = {0, 0, 0, 0, 0, 0}, cc[6] = {0, 0, 0, 0, 0, 0}, b = 0, g = 0;
        for (int s = D.incp[k]; s < D.incp[k + 1]; s++) {
            const int e = D.inc[s] >> 1, side = D.inc[s] & 1;
            const double *J = D.J + 72 * (size_t)e + 36 * side, *r = D.r + 6 * (size_t)e;
#pragma unroll
            for (int q = 0; q < 6; q++) {
                const double jc = J[6 * q + c], js = jc * sc;
                g += jc * r[q];
                b += js * r[q];
#pragma unroll
                for (int a = 0; a < 6; a++) h[a] += (J[6 * q + a] * sk[a]) * js;
            }
        }
        // coupling to the next variable pose: the entries of pose k + 1 whose other end is pose k
        if (k + 1 < D.n_var)
            for (int s = D.incp[k + 1]; s < D.incp[k + 2]; s++) {
                const int e = D.inc[s] >> 1, side = D.inc[s] & 1;
                const int other = side ? D.ei[e] : D.ej[e];
                if (D.vidx[other] != k) continue;
                const double *Jn = D.J + 72 * (size_t)e + 36 * side, *Jk = D.J + 72 * (size_t)e + 36 * (1 - side);
                const double sn = D.scale[6 * (k + 1) + c];
#pragma unroll
                for (int q = 0; q < 6; q++) {
                    const double js = Jn[6 * q + c] * sn;
#pragma unroll
                    for (int a = 0; a < 6; a++) cc[a] += (Jk[6 * q + a] * sk[a]) * js;
                }
            }
#pragma unroll
        for (int a = 0; a < 6; a++) { D.H[36 * (size_t)k + 6 * a + c] = h[a]; D.C[36 * (size_t)k + 6 * a + c] = cc[a]; }
        D.b[t] = b; D.g[t] = g;
    }
}

// in-place lower Cholesky of the 6x6 A (row-major, lower triangle read); false on a non-positive or non-finite pivot
__device__ __forceinline__ bool pg_chol6(double *A)
{
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double d = A[6 * j + j];
#pragma unroll
        for (int p = 0; p < j; p++) d -= A[6 * j + p] * A[6 * j + p];
        ok = ok && d > 0.0 && isfinite(d);
        const double l = sqrt(d);
        A[6 * j + j] = l;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double s = A[6 * i + j];
#pragma unroll
            for (int p = 0; p < j; p++) s -= A[6 * i + p] * A[6 * j + p];
            A[6 * i + j] = s / l;
        }
    }
    return ok;
}

// v <- L^-1 v
__device__ __forceinline__ void pg_fwd6(const double *L, double *v)
{
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double s = v[i];
#pragma unroll
        for (int p = 0; p < i; p++) s -= L[6 * i + p] * v[p];
        v[i] = s / L[6 * i + i];
    }
}

// v <- L^-T v
__device__ __forceinline__ void pg_bwd6(const double *L, double *v)
{
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        double s = v[i];
#pragma unroll
        for (int p = i + 1; p < 6; p++) s -= L[6 * p + i] * v[p];
        v[i] = s / L[6 * i + i];
    }
}

// (H + D^2) y = b along the variable poses [k0, k1): block Cholesky L_k L_k^T = A_k - W_{k-1}^T W_{k-1}, W_k = L_k^-1 C_k.
// D^2 = clamp(diag H) / radius.  Returns false when a pivot fails.
__device__ __forceinline__ bool pg_solve_segment(const PgDev &D, const BAOpt &O, double radius, int k0, int k1)
{
    double W[36], z[6];
    for (int k = k0; k < k1; k++) {
        double A[36], v[6];
        const double *H = D.H + 36 * (size_t)k;
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = 0; j <= i; j++) A[6 * i + j] = H[6 * i + j];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            const double d = sqrt(fmin(fmax(A[7 * i], O.min_diag), O.max_diag) / radius);
            A[7 * i] += d * d;
            v[i] = D.b[6 * k + i];
        }
        if (k > k0) {
#pragma unroll
            for (int i = 0; i < 6; i++) {
#pragma unroll
                for (int j = 0; j <= i; j++) {
                    double s = 0;
#pragma unroll
                    for (int p = 0; p < 6; p++) s += W[6 * p + i] * W[6 * p + j];
                    A[6 * i + j] -= s;
                }
                double s = 0;
#pragma unroll
                for (int p = 0; p < 6; p++) s += W[6 * p + i] * z[p];
                v[i] -= s;
            }
        }
        if (!pg_chol6(A)) return false;
        pg_fwd6(A, v);
        double *Lo = D.L + 36 * (size_t)k;
#pragma unroll
        for (int i = 0; i < 6; i++) {
            z[i] = v[i];
            D.y[6 * k + i] = v[i];
#pragma unroll
            for (int j = 0; j <= i; j++) Lo[6 * i + j] = A[6 * i + j];
        }
        if (k + 1 < k1) {
            const double *C = D.C + 36 * (size_t)k;
            double *Wo = D.W + 36 * (size_t)k;
#pragma unroll
            for (int c = 0; c < 6; c++) {
                double col[6];
#pragma unroll
                for (int i = 0; i < 6; i++) col[i] = C[6 * i + c];
                pg_fwd6(A, col);
#pragma unroll
                for (int i = 0; i < 6; i++) { W[6 * i + c] = col[i]; Wo[6 * i + c] = col[i]; }
            }
        }
    }
    double yn[6];
    for (int k = k1 - 1; k >= k0; k--) {
        double L[36], v[6];
        const double *Li = D.L + 36 * (size_t)k;
#pragma unroll
        for (int i = 0; i < 6; i++) {
            v[i] = D.y[6 * k + i];
#pragma unroll
            for (int j = 0; j <= i; j++) L[6 * i + j] = Li[6 * i + j];
        }
        if (k + 1 < k1) {
            const double *Wi = D.W + 36 * (size_t)k;
#pragma unroll
            for (int i = 0; i < 6; i++) {
                double s = 0;
#pragma unroll
                for (int p = 0; p < 6; p++) s += Wi[6 * i + p] * yn[p];
                v[i] -= s;
            }
        }
        pg_bwd6(L, v);
#pragma unroll
        for (int i = 0; i < 6; i++) { yn[i] = v[i]; D.y[6 * k + i] = v[i]; }
    }
    return true;
}

// A long segment [k0, k1) by the whole work-group: block cyclic reduction, ceil(log2 n) levels instead of n dependent steps.
// Rows are the variable poses of the segment; at stride s the rows that are odd multiples of s are eliminated,
//   x_i = h_i - G_i x_{i-s} - K_i x_{i+s},   h = A_i^-1 b_i,  G = A_i^-1 U_{i-s}^T,  K = A_i^-1 U_i   (phase 1, a lane per odd row)
// and the even multiples take the Schur complements (phase 2, a lane per even row)
//   A_e -= U_{e-s}^T K_{e-s} + U_e G_{e+s},   b_e -= U_{e-s}^T h_{e-s} + U_e h_{e+s},   U_e = -U_e K_{e+s}.
// Working copies: L holds A = H + D^2, W the couplings U, y the right-hand side and then the solution; G and K stay for the back
// substitution.  Every row is written by one lane per phase, in a fixed order.  Returns 1 in a lane that met a failed pivot.
__device__ __forceinline__ double pg_cr_segment(const PgDev &D, const BAOpt &O, double radius, int k0, int k1)
{
    const int n = k1 - k0, tid = threadIdx.x, nt = blockDim.x;
    double bad = 0;
    for (int t = tid; t < 36 * n; t += nt) {
        const size_t at = 36 * (size_t)k0 + t;
        const int e = t % 36;
        double a = D.H[at];
        if (e % 7 == 0) { const double d = sqrt(fmin(fmax(a, O.min_diag), O.max_diag) / radius); a += d * d; }
        D.L[at] = a;
        D.W[at] = D.C[at];
    }
    for (int t = tid; t < 6 * n; t += nt) D.y[6 * (size_t)k0 + t] = D.b[6 * (size_t)k0 + t];
    __syncthreads();
    int s = 1;
    for (; s < n; s <<= 1) {
        for (int m = tid; (2 * m + 1) * s < n; m += nt) {
            const int i = (2 * m + 1) * s;
            const size_t k = (size_t)(k0 + i), kp = k - s;
            const bool has_next = i + s < n;
            double A[36], v[6];
#pragma unroll
            for (int a = 0; a < 6; a++) {
                v[a] = D.y[6 * k + a];
#pragma unroll
                for (int c = 0; c <= a; c++) A[6 * a + c] = D.L[36 * k + 6 * a + c];
            }
            if (!pg_chol6(A)) bad = 1;
            pg_fwd6(A, v); pg_bwd6(A, v);
#pragma unroll
            for (int a = 0; a < 6; a++) D.y[6 * k + a] = v[a];
#pragma unroll 1
            for (int c = 0; c < 6; c++) {                  // (a column at a time: twelve interleaved solves would not fit the registers)
                double col[6];
#pragma unroll
                for (int a = 0; a < 6; a++) col[a] = D.W[36 * kp + 6 * c + a];                 // column c of U_{i-s}^T
                pg_fwd6(A, col); pg_bwd6(A, col);
#pragma unroll
                for (int a = 0; a < 6; a++) D.G[36 * k + 6 * a + c] = col[a];
            }
            if (has_next)
#pragma unroll 1
                for (int c = 0; c < 6; c++) {
                    double col[6];
#pragma unroll
                    for (int a = 0; a < 6; a++) col[a] = D.W[36 * k + 6 * a + c];
                    pg_fwd6(A, col); pg_bwd6(A, col);
#pragma unroll
                    for (int a = 0; a < 6; a++) D.K[36 * k + 6 * a + c] = col[a];
                }
        }
        __syncthreads();
        for (int m = tid; 2 * m * s < n; m += nt) {
            const int e = 2 * m * s;
            const size_t k = (size_t)(k0 + e);
            const bool has1 = m > 0, has2 = e + s < n, has3 = e + 2 * s < n;
            const size_t ka = has1 ? k - s : k, kb = has2 ? k + s : k;                                  // rows e - s and e + s where they exist
            const double *U1 = D.W + 36 * ka, *K1 = D.K + 36 * ka, *h1 = D.y + 6 * ka;
            const double *G2 = D.G + 36 * kb, *K2 = D.K + 36 * kb, *h2 = D.y + 6 * kb;
#pragma unroll 1
            for (int a = 0; a < 6; a++) {                  // a row of A_e, b_e and U_e at a time: little state in registers
                double A[6], U[6], Un[6], v = D.y[6 * k + a];
#pragma unroll
                for (int c = 0; c < 6; c++) { A[c] = D.L[36 * k + 6 * a + c]; U[c] = D.W[36 * k + 6 * a + c]; Un[c] = 0; }
                if (has1) {
#pragma unroll
                    for (int c = 0; c < 6; c++) {
                        double t = 0;
#pragma unroll
                        for (int p = 0; p < 6; p++) t += U1[6 * p + a] * K1[6 * p + c];
                        A[c] -= t;
                    }
                    double t = 0;
#pragma unroll
                    for (int p = 0; p < 6; p++) t += U1[6 * p + a] * h1[p];
                    v -= t;
                }
                if (has2) {
#pragma unroll
                    for (int c = 0; c < 6; c++) {
                        double t = 0;
#pragma unroll
                        for (int p = 0; p < 6; p++) t += U[p] * G2[6 * p + c];
                        A[c] -= t;
                    }
                    double t = 0;
#pragma unroll
                    for (int p = 0; p < 6; p++) t += U[p] * h2[p];
                    v -= t;
                    if (has3)
#pragma unroll
                        for (int c = 0; c < 6; c++) {
                            double u = 0;
#pragma unroll
                            for (int p = 0; p < 6; p++) u += U[p] * K2[6 * p + c];
                            Un[c] = -u;
                        }
                }
                D.y[6 * k + a] = v;
#pragma unroll
                for (int c = 0; c < 6; c++) {
                    if (c <= a) D.L[36 * k + 6 * a + c] = A[c];    // (the factorisation reads the lower triangle)
                    if (has3) D.W[36 * k + 6 * a + c] = Un[c];
                }
            }
        }
        __syncthreads();
    }
    if (tid == 0) {                                        // the last row
        const size_t k = (size_t)k0;
        double A[36], v[6];
#pragma unroll
        for (int a = 0; a < 6; a++) {
            v[a] = D.y[6 * k + a];
#pragma unroll
            for (int c = 0; c <= a; c++) A[6 * a + c] = D.L[36 * k + 6 * a + c];
        }
        if (!pg_chol6(A)) bad = 1;
        pg_fwd6(A, v); pg_bwd6(A, v);
#pragma unroll
        for (int a = 0; a < 6; a++) D.y[6 * k + a] = v[a];
    }
    __syncthreads();
    for (s >>= 1; s >= 1; s >>= 1) {
        for (int m = tid; (2 * m + 1) * s < n; m += nt) {
            const int i = (2 * m + 1) * s;
            const size_t k = (size_t)(k0 + i);
            const bool has_next = i + s < n;
            const double *G = D.G + 36 * k, *K = D.K + 36 * k, *xp = D.y + 6 * (k - s), *xn = D.y + 6 * (has_next ? k + s : k);
            double v[6];
#pragma unroll
            for (int a = 0; a < 6; a++) {
                double t = 0;
#pragma unroll
                for (int p = 0; p < 6; p++) t += G[6 * a + p] * xp[p];
                if (has_next)
#pragma unroll
                    for (int p = 0; p < 6; p++) t += K[6 * a + p] * xn[p];
                v[a] = D.y[6 * k + a] - t;
            }
#pragma unroll
            for (int a = 0; a < 6; a++) D.y[6 * k + a] = v[a];
        }
        __syncthreads();
    }
    return bad;
}

// cost, Jacobians, normal blocks and gradient at x: "a fresh linearisation" for the next d_ctl_iter_begin
__device__ __forceinline__ void pg_linearize(const PgDev &D, BACtl &cl, double *sh)
{
    const double cost = block_sum(pg_evaluate<true>(D, D.x), sh);
    if (threadIdx.x == 0) { cl.cost_acc = cost; cl.need_lin = 0; cl.fresh_lin = 1; }
    __syncthreads();                                       // r and J of every edge are in HBM
    pg_assemble(D);
    __syncthreads();
}

__global__ __launch_bounds__(PG_THREADS) void k_pg_solve(PgArgs a)
{
    __shared__ double sh[16];
    __shared__ BACtl cl;                                   // the trust-region state: thread 0 runs the d_ctl_* rules, every thread reads the verdict
    const PgItem it = a.items[blockIdx.x];
    if (it.n_act == 0) return;                             // nothing to optimise: the host has answered
    const BAOpt &O = a.O;
    const int tid = threadIdx.x, nt = blockDim.x;
    uint8_t *m = a.arena;
    PgDev D;
    D.n_poses = it.n_poses; D.n_var = it.n_var; D.n_act = it.n_act; D.n_seg = it.n_seg;
    D.x = (double *)(m + it.o_x); D.cand = (double *)(m + it.o_cand);
    D.vidx = (const int *)(m + it.o_vidx); D.ei = (const int *)(m + it.o_ei); D.ej = (const int *)(m + it.o_ej);
    D.incp = (const int *)(m + it.o_incp); D.inc = (const int *)(m + it.o_inc); D.seg = (const int *)(m + it.o_seg); D.vpose = D.seg + 2 * it.n_seg;
    D.eT = (const double *)(m + it.o_eT); D.esi = (const double *)(m + it.o_esi);
    D.r = (double *)(m + it.o_r); D.J = (double *)(m + it.o_J); D.H = (double *)(m + it.o_H); D.C = (double *)(m + it.o_C);
    D.g = (double *)(m + it.o_g); D.b = (double *)(m + it.o_b); D.scale = (double *)(m + it.o_scale); D.y = (double *)(m + it.o_y);
    D.L = (double *)(m + it.o_L); D.W = (double *)(m + it.o_W); D.G = (double *)(m + it.o_G); D.K = (double *)(m + it.o_K);

    for (int c = tid; c < 7 * D.n_poses; c += nt) D.cand[c] = D.x[c];
    for (int c = tid; c < 6 * D.n_var; c += nt) D.scale[c] = 1.0;
    __syncthreads();
    // a variable pose is in the program when an edge touches it
    auto in_program = [&](int k) { return D.incp[k] != D.incp[k + 1]; };
    auto grad_max = [&]() {
        double g = 0;
        for (int t = tid; t < 6 * D.n_var; t += nt) if (in_program(t / 6)) g = fmax(g, fabs(D.g[t]));
        return pg_block_max(g, sh);
    };
    // iteration 0
    if (tid == 0) ba_ctl_init(cl, a.initial_radius, a.trace);
    pg_linearize(D, cl, sh);
    if (O.jacobi) {
        for (int t = tid; t < 6 * D.n_var; t += nt) D.scale[t] = 1.0 / (1.0 + sqrt(D.H[36 * (size_t)(t / 6) + 7 * (t % 6)]));
        __syncthreads();
        pg_assemble(D);                                    // the blocks of the scaled Jacobian
        __syncthreads();
    }
    double gmax = grad_max();

    for (;;) {
        __syncthreads();                                   // every thread has read the last verdict
        if (tid == 0) d_ctl_iter_begin(cl, O, cl.fresh_lin, gmax);
        __syncthreads();
        if (cl.done) break;
        const double radius = cl.radius;
        double bad = 0;
        // short segments side by side, a lane each; long ones one after the other, the work-group on each
        for (int s = tid; s < D.n_seg; s += nt)
            if (D.seg[2 * s + 1] - D.seg[2 * s] < PG_CR_MIN && !pg_solve_segment(D, O, radius, D.seg[2 * s], D.seg[2 * s + 1])) bad = 1;
        for (int s = 0; s < D.n_seg; s++)
            if (D.seg[2 * s + 1] - D.seg[2 * s] >= PG_CR_MIN) bad = fmax(bad, pg_cr_segment(D, O, radius, D.seg[2 * s], D.seg[2 * s + 1]));
        for (int t = tid; t < 6 * D.n_var; t += nt) if (!in_program(t / 6)) D.y[t] = 0;      // (their segments were not listed)
        __syncthreads();
        // the step is -y; model cost change -(J s).(r + J s / 2) over the edges
        double mcc = 0;
        for (int e = tid; e < D.n_act; e += nt) {
            const int ki = D.vidx[D.ei[e]], kj = D.vidx[D.ej[e]];
            const double *J = D.J + 72 * (size_t)e, *r = D.r + 6 * (size_t)e;
            for (int q = 0; q < 6; q++) {
                double ms = 0;
                if (ki >= 0) for (int c = 0; c < 6; c++) ms += (J[6 * q + c] * D.scale[6 * ki + c]) * -D.y[6 * ki + c];
                if (kj >= 0) for (int c = 0; c < 6; c++) ms += (J[36 + 6 * q + c] * D.scale[6 * kj + c]) * -D.y[6 * kj + c];
                mcc -= ms * (r[q] + ms / 2.0);
            }
        }
        for (int t = tid; t < 6 * D.n_var; t += nt) if (!isfinite(D.y[t])) bad = 1;
        const bool lin_ok = pg_block_max(bad, sh) == 0;
        mcc = block_sum(mcc, sh);
        if (tid == 0) { if (!lin_ok) cl.lin_fail = 1; d_ctl_candidate(cl, O, lin_ok, mcc); }
        __syncthreads();
        if (cl.done) break;
        if (!cl.step_valid) continue;
        double step_sq = 0, xn = 0;
        for (int k = tid; k < D.n_var; k += nt) {
            if (!in_program(k)) continue;
            const int p = D.vpose[k];
            double delta[6], out[7];
            for (int c = 0; c < 6; c++) delta[c] = -D.y[6 * k + c] * D.scale[6 * k + c];
            pg_se3_left_plus(D.x + 7 * p, delta, out);
            for (int c = 0; c < 7; c++) {
                const double xv = D.x[7 * p + c];
                D.cand[7 * p + c] = out[c];
                step_sq += (xv - out[c]) * (xv - out[c]); xn += out[c] * out[c];
            }
        }
        __syncthreads();
        const double cand_cost = block_sum(pg_evaluate<false>(D, D.cand), sh);
        step_sq = block_sum(step_sq, sh);
        xn = block_sum(xn, sh);
        if (tid == 0) { cl.cost_acc = cand_cost; d_ctl_decide(cl, O, step_sq, xn); }
        __syncthreads();
        if (cl.done) break;
        if (cl.step_successful) {
            for (int k = tid; k < D.n_var; k += nt) if (in_program(k)) {
                const int p = D.vpose[k];
                for (int c = 0; c < 7; c++) D.x[7 * p + c] = D.cand[7 * p + c];
            }
            __syncthreads();
            pg_linearize(D, cl, sh);
            gmax = grad_max();
        }
    }
    if (tid == 0) {
        PgOut &o = a.out[blockIdx.x];
        // the run of invalid steps ended on a failed factorisation: Ceres' FAILURE, the solution is not usable
        const bool failed = cl.termination == OV2_TERM_INVALID_STEPS && cl.lin_fail;
        o.iterations = cl.n_steps; o.num_successful_steps = cl.n_success; o.termination = failed ? OV2_TERM_FAILURE : cl.termination;
        o.n_trace = cl.n_trace; o.initial_cost = cl.initial_cost; o.final_cost = cl.minimum_cost;
    }
}

// ---------------------------------------------------------------------------------- the rigid moves after the solve
struct PgApply {
    int n_win, n_young, n_pts;
    const double *win_old, *win_new, *young_old, *xyz;
    const int *pt_kf;
    double *young_new, *xyz_out;
    double ini_Tcw[7], newopt_Twc[7];
};

__device__ __forceinline__ PgSE3 pg_young(const PgApply &a, int k)
{
    return pg_mul(pg_load(a.newopt_Twc), pg_mul(pg_load(a.ini_Tcw), pg_load(a.young_old + 7 * (size_t)k)));
}

// lanes [0, n_young): a younger keyframe; lanes [n_young, n_young + n_pts): a point
__global__ __launch_bounds__(256) void k_pg_apply(PgApply a)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < a.n_young) {
        const PgSE3 T = pg_young(a, (int)t);
        double *o = a.young_new + 7 * t;
        o[0] = T.t[0]; o[1] = T.t[1]; o[2] = T.t[2]; o[3] = T.q[0]; o[4] = T.q[1]; o[5] = T.q[2]; o[6] = T.q[3];
        return;
    }
    const long long i = t - a.n_young;
    if (i >= a.n_pts) return;
    const int kf = a.pt_kf[i];
    PgSE3 Told, Tnew;
    if (kf < a.n_win) { Told = pg_load(a.win_old + 7 * (size_t)kf); Tnew = pg_load(a.win_new + 7 * (size_t)kf); }
    else { Told = pg_load(a.young_old + 7 * (size_t)(kf - a.n_win)); Tnew = pg_young(a, kf - a.n_win); }
    const PgSE3 Tcw = pg_inv(Told);
    const double X[3] = {a.xyz[3 * i], a.xyz[3 * i + 1], a.xyz[3 * i + 2]};
    double c[3], w[3];
    pg_rot(Tcw.q, X, c);
    c[0] += Tcw.t[0]; c[1] += Tcw.t[1]; c[2] += Tcw.t[2];
    pg_rot(Tnew.q, c, w);
    a.xyz_out[3 * i] = w[0] + Tnew.t[0]; a.xyz_out[3 * i + 1] = w[1] + Tnew.t[1]; a.xyz_out[3 * i + 2] = w[2] + Tnew.t[2];
}

// ---------------------------------------------------------------------------------- host
static bool pg_pose_ok(const double *p)
{
    for (int k = 0; k < 7; k++) if (!std::isfinite(p[k])) return false;
    return true;
}
static bool pg_quat_ok(const double *p) { return p[3] * p[3] + p[4] * p[4] + p[5] * p[5] + p[6] * p[6] > 0.0; }

// what the host derives from one problem
struct PgHost {
    std::vector<int> vidx, vpose, ei, ej, incp, inc, seg, src;      // src: caller's index of each active edge
    int n_var = 0, n_act = 0, n_seg = 0;
};

// validates one problem and builds its tables; no device work
static int pg_prepare(const ov2_pg_problem &p, const ov2_pg_result &r, PgHost &h)
{
    OV2_REQUIRE(p.n_poses >= 0 && p.n_edges >= 0, OV2_EINVAL, "negative count (n_poses / n_edges)");
    OV2_REQUIRE(p.n_poses <= OV2_PG_MAX_POSES, OV2_EINVAL, "capacity: more than 16384 poses in one problem");
    OV2_REQUIRE(p.n_edges <= OV2_PG_MAX_EDGES, OV2_EINVAL, "capacity: more than 32768 edges in one problem");
    OV2_REQUIRE(p.n_poses == 0 || (p.poses && p.pose_const), OV2_EINVAL, "NULL poses / pose_const");
    OV2_REQUIRE(p.n_edges == 0 || (p.edge_i && p.edge_j && p.edge_T), OV2_EINVAL, "NULL edge_i / edge_j / edge_T");
    OV2_REQUIRE(p.n_poses == 0 || r.poses_out, OV2_EINVAL, "NULL result buffer (poses_out)");
    for (int i = 0; i < p.n_poses; i++) {
        OV2_REQUIRE(pg_pose_ok(p.poses + 7 * (size_t)i), OV2_EINVAL, "pose not finite");
        OV2_REQUIRE(pg_quat_ok(p.poses + 7 * (size_t)i), OV2_EINVAL, "pose with a zero quaternion");
    }
    h.vidx.assign((size_t)p.n_poses + 1, -1);
    h.vpose.clear();
    for (int i = 0; i < p.n_poses; i++) if (!p.pose_const[i]) { h.vidx[i] = (int)h.vpose.size(); h.vpose.push_back(i); }
    h.n_var = (int)h.vpose.size();
    h.ei.clear(); h.ej.clear(); h.src.clear();
    std::vector<uint8_t> coupled((size_t)h.n_var + 1, 0);
    for (int e = 0; e < p.n_edges; e++) {
        const int i = p.edge_i[e], j = p.edge_j[e];
        OV2_REQUIRE(i >= 0 && i < p.n_poses && j >= 0 && j < p.n_poses, OV2_EINVAL, "edge index out of range");
        OV2_REQUIRE(i != j, OV2_EINVAL, "edge with i == j");
        OV2_REQUIRE(pg_pose_ok(p.edge_T + 7 * (size_t)e), OV2_EINVAL, "edge measurement not finite");
        OV2_REQUIRE(pg_quat_ok(p.edge_T + 7 * (size_t)e), OV2_EINVAL, "edge measurement with a zero quaternion");
        if (p.edge_sigma) OV2_REQUIRE(std::isfinite(p.edge_sigma[e]) && p.edge_sigma[e] > 0.0, OV2_EINVAL, "edge_sigma <= 0 or not finite");
        const int ki = h.vidx[i], kj = h.vidx[j];
        if (ki < 0 && kj < 0) continue;                    // two constant ends: not in the program
        if (ki >= 0 && kj >= 0) {
            if (ki - kj != 1 && kj - ki != 1) {
                ov2_set_error("%s:%d: edge %d (%d, %d) joins two variable poses that are not neighbours among the variable poses: "
                              "the normal matrix would not be block-tridiagonal", __FILE__, __LINE__, e, i, j);
                return OV2_EUNSUPPORTED;
            }
            coupled[ki < kj ? ki : kj] = 1;
        }
        h.ei.push_back(i); h.ej.push_back(j); h.src.push_back(e);
    }
    h.n_act = (int)h.ei.size();
    // pose -> incident (edge, side) entries, in edge order
    h.incp.assign((size_t)h.n_var + 2, 0);
    for (int e = 0; e < h.n_act; e++) {
        if (h.vidx[h.ei[e]] >= 0) h.incp[h.vidx[h.ei[e]] + 1]++;
        if (h.vidx[h.ej[e]] >= 0) h.incp[h.vidx[h.ej[e]] + 1]++;
    }
    for (int k = 0; k < h.n_var; k++) h.incp[k + 1] += h.incp[k];
    h.inc.assign((size_t)h.incp[h.n_var] + 1, 0);
    {
        std::vector<int> fill(h.incp.begin(), h.incp.end());
        for (int e = 0; e < h.n_act; e++) {
            if (h.vidx[h.ei[e]] >= 0) h.inc[fill[h.vidx[h.ei[e]]]++] = 2 * e;
            if (h.vidx[h.ej[e]] >= 0) h.inc[fill[h.vidx[h.ej[e]]]++] = 2 * e + 1;
        }
    }
    // segments: runs of in-program variable poses joined by edges, as (first, end) pairs
    h.seg.clear();
    for (int k = 0; k < h.n_var; k++) {
        if (h.incp[k] == h.incp[k + 1]) continue;          // no edge: not in the program
        if (k > 0 && coupled[k - 1]) continue;             // inside a segment
        int end = k;
        while (coupled[end]) end++;
        h.seg.push_back(k); h.seg.push_back(end + 1);
    }
    h.n_seg = (int)h.seg.size() / 2;
    return OV2_OK;
}

static int pg_check_options(const ov2_ba_options *o)
{
    OV2_REQUIRE(o->max_iter >= 0, OV2_EINVAL, "max_iter < 0");
    OV2_REQUIRE(!(o->huber_delta > 0.0), OV2_EUNSUPPORTED, "huber_delta > 0: the pose-graph solver has no loss function (the reference passes none)");
    OV2_REQUIRE(!(o->max_solver_time_s > 0.0), OV2_EUNSUPPORTED,
                "max_solver_time_s > 0: the pose-graph loop runs inside one launch and cannot honour a time limit");
    OV2_REQUIRE(std::isfinite(o->initial_radius) && o->initial_radius > 0.0, OV2_EINVAL, "initial_radius <= 0 or not finite");
    return OV2_OK;
}

extern "C" {

int ov2_pose_graph_solve_batch(ov2_ctx *ctx, int n_items, const ov2_pg_problem *p, const ov2_ba_options *opt, ov2_pg_result *res)
{
    // the inputs first, the context last: a malformed input is reported without a device
    OV2_REQUIRE(opt, OV2_EINVAL, "NULL options");
    OV2_REQUIRE(n_items >= 0, OV2_EINVAL, "n_items < 0");
    OV2_REQUIRE(n_items == 0 || (p && res), OV2_EINVAL, "NULL problem / result array");
    OV2_REQUIRE(n_items <= 65535, OV2_EINVAL, "more than 65535 problems in one call");
    int rc = pg_check_options(opt);  if (rc) return rc;
    std::vector<PgHost> H((size_t)n_items);
    for (int b = 0; b < n_items; b++) { rc = pg_prepare(p[b], res[b], H[b]); if (rc) return rc; }
    OV2_REQUIRE(ctx, OV2_EINVAL, "NULL context");
    if (n_items == 0) return OV2_OK;

    // arena: [items][out][x of every item] [the other staged arrays] [workspace]; up: everything before the workspace, down: out and x
    const size_t B = (size_t)n_items;
    std::vector<PgItem> items(B);
    StageCursor c(16);
    c.take(sizeof(PgItem) * B);
    const size_t o_out = c.take(sizeof(PgOut) * B);
    bool any = false;
    for (size_t b = 0; b < B; b++) {
        PgItem &it = items[b];
        it.n_poses = p[b].n_poses; it.n_var = H[b].n_var; it.n_act = H[b].n_act; it.n_seg = H[b].n_seg;
        it.o_x = c.take(56 * (size_t)it.n_poses);
        any = any || it.n_act > 0;
    }
    const size_t down_end = c.off;
    for (size_t b = 0; b < B; b++) {
        PgItem &it = items[b];
        const size_t NP = (size_t)it.n_poses + 1, NV = (size_t)it.n_var + 2, NE = (size_t)it.n_act + 1;
        it.o_vidx = c.take(4 * NP); it.o_ei = c.take(4 * NE); it.o_ej = c.take(4 * NE); it.o_eT = c.take(56 * NE); it.o_esi = c.take(8 * NE);
        it.o_incp = c.take(4 * NV); it.o_inc = c.take(4 * (H[b].inc.size() + 1)); it.o_seg = c.take(4 * (2 * (size_t)it.n_seg + NV));
    }
    const size_t up_end = c.off;
    for (size_t b = 0; b < B; b++) {
        PgItem &it = items[b];
        const size_t NP = (size_t)it.n_poses + 1, NV = (size_t)it.n_var + 1, NE = (size_t)it.n_act + 1;
        it.o_cand = c.take(56 * NP); it.o_r = c.take(48 * NE); it.o_J = c.take(576 * NE);
        it.o_H = c.take(288 * NV); it.o_C = c.take(288 * NV); it.o_L = c.take(288 * NV); it.o_W = c.take(288 * NV); it.o_G = c.take(288 * NV); it.o_K = c.take(288 * NV);
        it.o_g = c.take(48 * NV); it.o_b = c.take(48 * NV); it.o_scale = c.take(48 * NV); it.o_y = c.take(48 * NV);
    }
    const size_t total = c.off;
    float ms = 0;
    const uint8_t *hs_c = nullptr;
    const bool trace = n_items == 1 && ctx->ba_trace;      // ov2_pose_graph_solve (a batch call with one item is the same call)
    BAIterRec *trace_d = nullptr;
    ctx->ba_trace_n = 0;                                   // (also when nothing is solved)
    if (any) {
        Stage st;
        rc = st.open(ctx, total, up_end);  if (rc) return rc;      // (the workspace stays on the device)
        rc = ba_trace_begin(ctx, trace, &trace_d);  if (rc) return rc;
        uint8_t *hs = st.h, *ds = st.d;
        memset(hs, 0, up_end);
        for (size_t b = 0; b < B; b++) {
            const PgItem &it = items[b];
            const PgHost &h = H[b];
            memcpy(hs + sizeof(PgItem) * b, &it, sizeof(PgItem));
            if (it.n_poses) {
                memcpy(hs + it.o_x, p[b].poses, 56 * (size_t)it.n_poses);
                memcpy(hs + it.o_vidx, h.vidx.data(), 4 * (size_t)it.n_poses);
            }
            if (it.n_act) { memcpy(hs + it.o_ei, h.ei.data(), 4 * (size_t)it.n_act); memcpy(hs + it.o_ej, h.ej.data(), 4 * (size_t)it.n_act); }
            for (int e = 0; e < it.n_act; e++) {
                memcpy(hs + it.o_eT + 56 * (size_t)e, p[b].edge_T + 7 * (size_t)h.src[e], 56);
                ((double *)(hs + it.o_esi))[e] = p[b].edge_sigma ? 1.0 / p[b].edge_sigma[h.src[e]] : 1.0;
            }
            memcpy(hs + it.o_incp, h.incp.data(), 4 * ((size_t)it.n_var + 1));
            if (h.incp[it.n_var]) memcpy(hs + it.o_inc, h.inc.data(), 4 * (size_t)h.incp[it.n_var]);
            if (it.n_seg) memcpy(hs + it.o_seg, h.seg.data(), 8 * (size_t)it.n_seg);
            if (it.n_var) memcpy(hs + it.o_seg + 8 * (size_t)it.n_seg, h.vpose.data(), 4 * (size_t)it.n_var);
        }
        rc = st.upload(0, up_end);  if (rc) return rc;
        PgArgs a;
        a.arena = ds; a.items = (const PgItem *)ds; a.out = (PgOut *)(ds + o_out);
        a.O = ba_opt_from(*opt); a.initial_radius = opt->initial_radius;
        a.trace = trace_d;
        rc = ba_events(ctx);  if (rc) return rc;
        OV2_HIP_CHECK(hipEventRecord(ctx->ba_ev[0], ctx->stream));
        hipLaunchKernelGGL(k_pg_solve, dim3(n_items), dim3(PG_THREADS), 0, ctx->stream, a);
        OV2_HIP_CHECK(hipGetLastError());
        OV2_HIP_CHECK(hipEventRecord(ctx->ba_ev[1], ctx->stream));
        rc = st.download(o_out, down_end, o_out);  if (rc) return rc;
        rc = st.sync();  if (rc) return rc;
        OV2_HIP_CHECK(hipEventElapsedTime(&ms, ctx->ba_ev[0], ctx->ba_ev[1]));
        hs_c = hs;
    }
    for (size_t b = 0; b < B; b++) {
        ov2_pg_result &r = res[b];
        const size_t bytes = 56 * (size_t)p[b].n_poses;
        r.solve_ms = ms;
        if (items[b].n_act == 0) {                         // Ceres: "no non-constant parameter blocks"
            if (bytes) memmove(r.poses_out, p[b].poses, bytes);
            r.iterations = 0; r.num_successful_steps = 0; r.initial_cost = 0.0; r.final_cost = 0.0; r.termination = OV2_TERM_FUNCTION_TOL;
            continue;
        }
        PgOut o;
        memcpy(&o, hs_c + o_out + sizeof(PgOut) * b, sizeof(PgOut));
        // an unusable solution is not written back: the input poses
        if (o.termination == OV2_TERM_FAILURE) memmove(r.poses_out, p[b].poses, bytes);
        else memcpy(r.poses_out, hs_c + items[b].o_x, bytes);
        r.iterations = o.iterations; r.num_successful_steps = o.num_successful_steps; r.initial_cost = o.initial_cost;
        r.final_cost = o.final_cost; r.termination = o.termination;
        if (trace) { rc = ba_trace_fetch(ctx, o.n_trace);  if (rc) return rc; }
    }
    return OV2_OK;
}

int ov2_pose_graph_solve(ov2_ctx *ctx, const ov2_pg_problem *p, const ov2_ba_options *opt, ov2_pg_result *res)
{
    OV2_REQUIRE(p && res, OV2_EINVAL, "NULL problem / result");
    return ov2_pose_graph_solve_batch(ctx, 1, p, opt, res);
}

int ov2_pose_graph_apply(ov2_ctx *ctx, int n_win, const double *win_old, const double *win_new, const double ini_Tcw[7],
                         const double newopt_Twc[7], int n_young, const double *young_old, double *young_new, int n_pts,
                         const double *xyz, const int *pt_kf, double *xyz_out)
{
    OV2_REQUIRE(n_win >= 0 && n_young >= 0 && n_pts >= 0, OV2_EINVAL, "negative count (n_win / n_young / n_pts)");
    OV2_REQUIRE(n_win <= (1 << 24) && n_young <= (1 << 24), OV2_EINVAL, "capacity: more than 2^24 keyframes");
    OV2_REQUIRE(n_pts <= (1 << 27), OV2_EINVAL, "capacity: more than 2^27 points");
    OV2_REQUIRE(n_win == 0 || (win_old && win_new), OV2_EINVAL, "NULL win_old / win_new");
    OV2_REQUIRE(n_young == 0 || (young_old && young_new && ini_Tcw && newopt_Twc), OV2_EINVAL, "NULL young_old / young_new / ini_Tcw / newopt_Twc");
    OV2_REQUIRE(n_pts == 0 || (xyz && pt_kf && xyz_out), OV2_EINVAL, "NULL xyz / pt_kf / xyz_out");
    OV2_REQUIRE(n_pts == 0 || n_win + n_young > 0, OV2_EINVAL, "points without a keyframe");
    auto poses_ok = [](const double *P, int n) {
        for (int i = 0; i < n; i++) if (!pg_pose_ok(P + 7 * (size_t)i) || !pg_quat_ok(P + 7 * (size_t)i)) return false;
        return true;
    };
    OV2_REQUIRE(poses_ok(win_old, n_win) && poses_ok(win_new, n_win) && poses_ok(young_old, n_young), OV2_EINVAL,
                "pose not finite or with a zero quaternion");
    OV2_REQUIRE(n_young == 0 || (poses_ok(ini_Tcw, 1) && poses_ok(newopt_Twc, 1)), OV2_EINVAL, "ini_Tcw / newopt_Twc not finite or with a zero quaternion");
    for (int i = 0; i < n_pts; i++) {
        OV2_REQUIRE(pt_kf[i] >= 0 && pt_kf[i] < n_win + n_young, OV2_EINVAL, "pt_kf out of range");
        OV2_REQUIRE(std::isfinite(xyz[3 * (size_t)i]) && std::isfinite(xyz[3 * (size_t)i + 1]) && std::isfinite(xyz[3 * (size_t)i + 2]), OV2_EINVAL, "xyz not finite");
    }
    OV2_REQUIRE(ctx, OV2_EINVAL, "NULL context");
    if (n_young + n_pts == 0) return OV2_OK;
    // staging: [win_old][win_new][young_old][xyz][pt_kf] up, [young_new][xyz_out] down
    const size_t W = 56 * (size_t)n_win, Y = 56 * (size_t)n_young, X = 24 * (size_t)n_pts;
    StageCursor c(16);
    const size_t o_wo = c.take(W), o_wn = c.take(W), o_yo = c.take(Y), o_x = c.take(X), o_kf = c.take(4 * (size_t)n_pts);
    const size_t o_yn = c.take(Y), o_xo = c.take(X), total = c.off;
    Stage st;
    int rc = st.open(ctx, total, total);  if (rc) return rc;
    uint8_t *hs = st.h, *ds = st.d;
    if (n_win) { memcpy(hs + o_wo, win_old, W); memcpy(hs + o_wn, win_new, W); }
    if (n_young) memcpy(hs + o_yo, young_old, Y);
    if (n_pts) { memcpy(hs + o_x, xyz, X); memcpy(hs + o_kf, pt_kf, 4 * (size_t)n_pts); }
    rc = st.upload(0, o_yn);  if (rc) return rc;
    PgApply a{};
    a.n_win = n_win; a.n_young = n_young; a.n_pts = n_pts;
    a.win_old = (const double *)(ds + o_wo); a.win_new = (const double *)(ds + o_wn); a.young_old = (const double *)(ds + o_yo);
    a.xyz = (const double *)(ds + o_x); a.pt_kf = (const int *)(ds + o_kf); a.young_new = (double *)(ds + o_yn); a.xyz_out = (double *)(ds + o_xo);
    for (int k = 0; k < 7; k++) { a.ini_Tcw[k] = n_young ? ini_Tcw[k] : (k == 6); a.newopt_Twc[k] = n_young ? newopt_Twc[k] : (k == 6); }
    const long long lanes = (long long)n_young + n_pts;
    hipLaunchKernelGGL(k_pg_apply, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, ctx->stream, a);
    OV2_HIP_CHECK(hipGetLastError());
    rc = st.download(o_yn, total, o_yn);  if (rc) return rc;
    rc = st.sync();  if (rc) return rc;
    if (n_young) memcpy(young_new, hs + o_yn, Y);
    if (n_pts) memcpy(xyz_out, hs + o_xo, X);
    return OV2_OK;
}

} // extern "C"
