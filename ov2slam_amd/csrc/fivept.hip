// fivept.hip -- relative pose from 2D-2D matches for gfx950 (the reference's MultiViewGeometry::compute5ptEssentialMatrix with
// USE_OPENGV, src/multi_view_geometry.cpp:594-696: CentralRelativePoseSacProblem::NISTER under sac::Ransac).  OpenGV is not available
// to this project: the solver and the loop are restated (tests/fivept_ref.py is the same specification in numpy), nothing is pinned
// against an OpenGV binary.  The sample table is an INPUT (eight indices per row), so a call is a deterministic function of its
// arguments:
//   k_e5_solve   ONE LANE PER (problem, row), 32 rows per work-group.  Everything that is indexed at run time lives in LDS, one
//                column of 236 doubles per lane laid out lane-minor (slot * 32 + lane: the lanes of a wavefront read consecutive
//                doubles, no bank conflict while they walk in step): the 5 x 9 matrix and its full-pivot Gauss-Jordan, the four
//                null vectors (modified Gram-Schmidt), the 10 x 20 constraint matrix and its partial-pivot Gauss-Jordan, then, over
//                the dead matrix, B(z), det B(z), the Sturm chain and the roots.  The polynomial algebra in (x, y, z) and the
//                products of B(z)'s entries are unrolled in registers.  Per root: x, y from the best 2 x 2 of B(z), Horn's closed
//                form for the four (R, t), the sum of e5_dist over the row's eight matches picks one.  Every trip count is bounded.
//   k_e5_score   ONE WAVEFRONT PER (problem, row), lanes striding over the points: inliers (e5_dist < threshold) by ballots.
//   k_e5_pick    ONE WAVEFRONT PER PROBLEM: lane 0 replays the sequential RANSAC loop over the per-row counts (skipped rows do not
//                count, a strictly larger count wins, the adaptive iteration bound with a sample size of 8), then all lanes classify
//                the points against the winner with the same e5_dist and write the ascending outlier list by ballot-prefix
//                compaction.
// No atomics, no result that depends on scheduling.  Every pointer and size is validated on the host before any device work; the
// solve kernel checks every sample index against the problem's point count before it reads through it.
#include "common.hpp"
#include "fivept_dev.hpp"              // E5Item, E5Out, E5Args and the host step (e5_enqueue) that epifilter.hip chains as well
#include <cmath>
#include <cfloat>

#pragma clang fp contract(off)

#define E5_MAX_POINTS 2048
#define E5_MAX_ROWS 4096
#define E5_LANES 32                    // hypotheses per work-group of k_e5_solve
#define E5_SLOTS 236                   // doubles of LDS per hypothesis: 200 (matrices; later B, det B, chain, roots) + 36 (null vectors)
#define E5_ISOLATE 40                  // tests/fivept_ref.py: ISOLATE_TRIPS, REFINE_TRIPS, NEWTON_STEPS
#define E5_REFINE 30
#define E5_NEWTON 3
#define E5_MIN_INLIERS 10              // src/multi_view_geometry.cpp:665
static_assert(E5_MAX_POINTS == OV2_EPI_MAX_POINTS && E5_MAX_ROWS == OV2_EPI_MAX_ROWS, "capacity");
static_assert(E5_SLOTS * E5_LANES * 8 <= 65536, "k_e5_solve: LDS per work-group");

struct E5V { double x, y, z; };
__device__ __forceinline__ E5V e5_cross(E5V a, E5V b) { return E5V{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double e5_dot(E5V a, E5V b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ E5V e5_load(const double *p, size_t i) { return E5V{p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
__device__ __forceinline__ bool e5_finite(double v) { return fabs(v) <= DBL_MAX; }
struct E5Model { double R[9]; E5V t; };            // x1 = R x2 + t, R row-major

// d = (1 - f1 . p / |p|) + (1 - f2 . r / |r|): p the midpoint of the two rays in frame 1 (opengv::triangulation::triangulate2 as
// csrc/triangulate.hip restates it in tri_triangulate2), r = R^T (p - t).  The ONE distance of the solve, the score and the pick.
__device__ __forceinline__ double e5_dist(const E5Model &m, E5V f1, E5V f2)
{
    const double *R = m.R;
    const E5V t = m.t;
    const E5V f2u{(R[0] * f2.x + R[1] * f2.y) + R[2] * f2.z, (R[3] * f2.x + R[4] * f2.y) + R[5] * f2.z, (R[6] * f2.x + R[7] * f2.y) + R[8] * f2.z};
    const double b0 = e5_dot(f1, t), b1 = e5_dot(f2u, t);
    const double a00 = e5_dot(f1, f1), a10 = e5_dot(f1, f2u);
    const double a01 = -a10, a11 = -e5_dot(f2u, f2u);
    const double invdet = 1. / (a00 * a11 - a10 * a01);
    const double i00 = a11 * invdet, i10 = -a10 * invdet, i01 = -a01 * invdet, i11 = a00 * invdet;
    const double l0 = i00 * b0 + i01 * b1, l1 = i10 * b0 + i11 * b1;
    const E5V p{(l0 * f1.x + (t.x + l1 * f2u.x)) / 2., (l0 * f1.y + (t.y + l1 * f2u.y)) / 2., (l0 * f1.z + (t.z + l1 * f2u.z)) / 2.};
    const E5V q{p.x - t.x, p.y - t.y, p.z - t.z};
    const E5V r{(q.x * R[0] + q.y * R[3]) + q.z * R[6], (q.x * R[1] + q.y * R[4]) + q.z * R[7], (q.x * R[2] + q.y * R[5]) + q.z * R[8]};
    return (1. - e5_dot(f1, p) / sqrt(e5_dot(p, p))) + (1. - e5_dot(f2, r) / sqrt(e5_dot(r, r)));
}

// ---- polynomials in (x, y, z): variables 0 = x, 1 = y, 2 = z, 3 = 1; monomials are sorted tuples in lexicographic order ----
__device__ __forceinline__ constexpr int e5_qidx(int i, int j) { return i * 4 - i * (i - 1) / 2 + (j - i); }               // i <= j
__device__ __forceinline__ constexpr int e5_cidx(int a, int b, int c)                                                       // a <= b <= c
{
    return (a == 0 ? 0 : (a == 1 ? 10 : (a == 2 ? 16 : 19))) + (b - a) * (4 - a) - (b - a) * (b - a - 1) / 2 + (c - b);
}
// q += a * b, two linear forms
__device__ __forceinline__ void e5_mul11(const double (&a)[4], const double (&b)[4], double (&q)[10])
{
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) q[e5_qidx(i < j ? i : j, i < j ? j : i)] += a[i] * b[j];
}
// c += q * l
__device__ __forceinline__ void e5_mul21(const double (&q)[10], const double (&l)[4], double (&c)[20])
{
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = i; j < 4; j++)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int lo = k < i ? k : i, hi = k > j ? k : j, mid = i + j + k - lo - hi;
                c[e5_cidx(lo, mid, hi)] += q[e5_qidx(i, j)] * l[k];
            }
}
// a (NA coefficients) times b (NB), highest power first
template <int NA, int NB>
__device__ __forceinline__ void e5_pmul(const double (&a)[NA], const double (&b)[NB], double (&o)[NA + NB - 1])
{
#pragma unroll
    for (int i = 0; i < NA + NB - 1; i++) o[i] = 0.;
#pragma unroll
    for (int i = 0; i < NA; i++)
#pragma unroll
        for (int j = 0; j < NB; j++) o[i + j] = o[i + j] + a[i] * b[j];
}

#define SM(i) sm[(i) * E5_LANES + lane]
#define A59(r, c) SM((r) * 9 + (c))
#define NV(j, e) SM(200 + (j) * 9 + (e))
#define M20(r, c) SM((r) * 20 + (c))
#define BZ(i) SM(i)                    // B(z): row r at 13 r: x (4), y (4), 1 (5)
#define PC(i) SM(39 + (i))             // det B(z), 11 coefficients
#define ST(k, i) SM(50 + (k) * 11 + (i))
#define RT(j) SM(171 + (j))

// sign changes along the Sturm chain at x; zeros and non-finite values are skipped
__device__ __forceinline__ int e5_sign_changes(const double *sm, int lane, double x)
{
    int n = 0, last = 0;
    for (int k = 0; k < 11; k++) {
        double v = ST(k, 0);
        for (int i = 1; i <= 10 - k; i++) v = v * x + ST(k, i);
        const int s = !e5_finite(v) ? 0 : (v > 0. ? 1 : (v < 0. ? -1 : 0));
        if (s != 0) {
            if (last != 0 && s != last) n++;
            last = s;
        }
    }
    return n;
}

__device__ __forceinline__ void e5_horner(const double *sm, int lane, double x, double &v, double &d)
{
    v = PC(0); d = 0.;
    for (int k = 1; k < 11; k++) { d = d * x + v; v = v * x + PC(k); }
}

__global__ __launch_bounds__(E5_LANES) void k_e5_solve(E5Args a)
{
    __shared__ double sm[E5_SLOTS * E5_LANES];
    const E5Item it = a.items[blockIdx.y];
    const int lane = threadIdx.x;
    const int r = blockIdx.x * E5_LANES + lane;
    if (r >= it.S) return;                                         // no barrier in this kernel: a lane owns its LDS column
    const size_t gr = (size_t)it.row0 + (size_t)r;
    const int4 s0 = a.samples[2 * gr], s1 = a.samples[2 * gr + 1];
    const int idx[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
    const unsigned n = (unsigned)it.n;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        ok = ok && (unsigned)idx[i] < n;
#pragma unroll
        for (int j = 0; j < i; j++) ok = ok && idx[i] != idx[j];
    }
    E5Model best{};
    bool have = false;
    const double *bv1 = a.bv1 + 3 * (size_t)it.pt0, *bv2 = a.bv2 + 3 * (size_t)it.pt0;
    if (ok) {
        // ---- 1-2: the 5 x 9 matrix, Gauss-Jordan with full pivoting, one null vector per free column, Gram-Schmidt ----
#pragma unroll
        for (int i = 0; i < 5; i++) {
            const E5V f1 = e5_load(bv1, idx[i]), f2 = e5_load(bv2, idx[i]);
            A59(i, 0) = f1.x * f2.x; A59(i, 1) = f1.x * f2.y; A59(i, 2) = f1.x * f2.z;
            A59(i, 3) = f1.y * f2.x; A59(i, 4) = f1.y * f2.y; A59(i, 5) = f1.y * f2.z;
            A59(i, 6) = f1.z * f2.x; A59(i, 7) = f1.z * f2.y; A59(i, 8) = f1.z * f2.z;
        }
        unsigned long long perm = 0x876543210ull;                  // column permutation, four bits per slot
        for (int k = 0; k < 5; k++) {
            int pr = k, pc = k;
            double big = -1.;
            for (int rr = k; rr < 5; rr++)
                for (int c = k; c < 9; c++) {
                    const double v = fabs(A59(rr, c));
                    if (v > big) { pr = rr; pc = c; big = v; }
                }
            if (pr != k)
                for (int c = 0; c < 9; c++) { const double t = A59(k, c); A59(k, c) = A59(pr, c); A59(pr, c) = t; }
            if (pc != k) {
                for (int rr = 0; rr < 5; rr++) { const double t = A59(rr, k); A59(rr, k) = A59(rr, pc); A59(rr, pc) = t; }
                const unsigned long long nk = (perm >> (4 * k)) & 15ull, np = (perm >> (4 * pc)) & 15ull;
                perm = (perm & ~((15ull << (4 * k)) | (15ull << (4 * pc)))) | (np << (4 * k)) | (nk << (4 * pc));
            }
            const double piv = A59(k, k);
            for (int c = k + 1; c < 9; c++) A59(k, c) = A59(k, c) / piv;
            A59(k, k) = 1.;
            for (int rr = 0; rr < 5; rr++) {
                if (rr == k) continue;
                const double f = A59(rr, k);
                for (int c = k + 1; c < 9; c++) A59(rr, c) = A59(rr, c) - f * A59(k, c);
                A59(rr, k) = 0.;
            }
        }
        for (int j = 0; j < 4; j++) {
            for (int e = 0; e < 9; e++) NV(j, e) = 0.;
            NV(j, (int)((perm >> (4 * (5 + j))) & 15ull)) = 1.;
            for (int i = 0; i < 5; i++) NV(j, (int)((perm >> (4 * i)) & 15ull)) = -A59(i, 5 + j);
        }
        for (int k = 0; k < 4; k++) {
            for (int j = 0; j < k; j++) {
                double d = 0.;
                for (int e = 0; e < 9; e++) d = d + NV(k, e) * NV(j, e);
                for (int e = 0; e < 9; e++) NV(k, e) = NV(k, e) - d * NV(j, e);
            }
            double s = 0.;
            for (int e = 0; e < 9; e++) s = s + NV(k, e) * NV(k, e);
            s = sqrt(s);
            for (int e = 0; e < 9; e++) NV(k, e) = NV(k, e) / s;
        }
        // ---- 3: (2 E E^T - tr(E E^T) I) E and det E as cubic forms, in Nister's monomial order ----
        {
            double e[9][4];
#pragma unroll
            for (int q = 0; q < 9; q++)
#pragma unroll
                for (int v = 0; v < 4; v++) e[q][v] = NV(v, q);
            double G[6][10];                                       // E E^T: (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = i; j < 3; j++) {
                    double (&g)[10] = G[i == 0 ? j : (i == 1 ? 2 + j : 5)];
#pragma unroll
                    for (int q = 0; q < 10; q++) g[q] = 0.;
                    double t1[10] = {}, t2[10] = {};
                    e5_mul11(e[3 * i], e[3 * j], g);
                    e5_mul11(e[3 * i + 1], e[3 * j + 1], t1);
                    e5_mul11(e[3 * i + 2], e[3 * j + 2], t2);
#pragma unroll
                    for (int q = 0; q < 10; q++) g[q] = (g[q] + t1[q]) + t2[q];
                }
            double tr[10];
#pragma unroll
            for (int q = 0; q < 10; q++) tr[q] = (G[0][q] + G[3][q]) + G[5][q];
#pragma unroll
            for (int i = 0; i < 3; i++) {
                double L[3][10];
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const int gi = i <= j ? (i == 0 ? j : (i == 1 ? 2 + j : 5)) : (j == 0 ? i : (j == 1 ? 2 + i : 5));
#pragma unroll
                    for (int q = 0; q < 10; q++) L[j][q] = i == j ? 2. * G[gi][q] - tr[q] : 2. * G[gi][q];
                }
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    double c0[20] = {}, c1[20] = {}, c2[20] = {};
                    e5_mul21(L[0], e[j], c0);
                    e5_mul21(L[1], e[3 + j], c1);
                    e5_mul21(L[2], e[6 + j], c2);
                    double c[20];
#pragma unroll
                    for (int q = 0; q < 20; q++) c[q] = (c0[q] + c1[q]) + c2[q];
                    const int row = 3 * i + j;
                    M20(row, 0) = c[0]; M20(row, 1) = c[10]; M20(row, 2) = c[1]; M20(row, 3) = c[4]; M20(row, 4) = c[2];
                    M20(row, 5) = c[3]; M20(row, 6) = c[11]; M20(row, 7) = c[12]; M20(row, 8) = c[5]; M20(row, 9) = c[6];
                    M20(row, 10) = c[7]; M20(row, 11) = c[8]; M20(row, 12) = c[9]; M20(row, 13) = c[13]; M20(row, 14) = c[14];
                    M20(row, 15) = c[15]; M20(row, 16) = c[16]; M20(row, 17) = c[17]; M20(row, 18) = c[18]; M20(row, 19) = c[19];
                }
            }
            {
                double m0[10] = {}, m1[10] = {}, c0[20] = {}, c1[20] = {}, c2[20] = {};
                e5_mul11(e[4], e[8], m0); e5_mul11(e[5], e[7], m1);
#pragma unroll
                for (int q = 0; q < 10; q++) m0[q] = m0[q] - m1[q];
                e5_mul21(m0, e[0], c0);
#pragma unroll
                for (int q = 0; q < 10; q++) { m0[q] = 0.; m1[q] = 0.; }
                e5_mul11(e[3], e[8], m0); e5_mul11(e[5], e[6], m1);
#pragma unroll
                for (int q = 0; q < 10; q++) m0[q] = m0[q] - m1[q];
                e5_mul21(m0, e[1], c1);
#pragma unroll
                for (int q = 0; q < 10; q++) { m0[q] = 0.; m1[q] = 0.; }
                e5_mul11(e[3], e[7], m0); e5_mul11(e[4], e[6], m1);
#pragma unroll
                for (int q = 0; q < 10; q++) m0[q] = m0[q] - m1[q];
                e5_mul21(m0, e[2], c2);
                double c[20];
#pragma unroll
                for (int q = 0; q < 20; q++) c[q] = (c0[q] - c1[q]) + c2[q];
                M20(9, 0) = c[0]; M20(9, 1) = c[10]; M20(9, 2) = c[1]; M20(9, 3) = c[4]; M20(9, 4) = c[2];
                M20(9, 5) = c[3]; M20(9, 6) = c[11]; M20(9, 7) = c[12]; M20(9, 8) = c[5]; M20(9, 9) = c[6];
                M20(9, 10) = c[7]; M20(9, 11) = c[8]; M20(9, 12) = c[9]; M20(9, 13) = c[13]; M20(9, 14) = c[14];
                M20(9, 15) = c[15]; M20(9, 16) = c[16]; M20(9, 17) = c[17]; M20(9, 18) = c[18]; M20(9, 19) = c[19];
            }
        }
        // Gauss-Jordan with partial pivoting on the first ten columns
        for (int k = 0; k < 10; k++) {
            int p = k;
            double big = -1.;
            for (int rr = k; rr < 10; rr++) {
                const double v = fabs(M20(rr, k));
                if (v > big) { p = rr; big = v; }
            }
            if (p != k)
                for (int c = 0; c < 20; c++) { const double t = M20(k, c); M20(k, c) = M20(p, c); M20(p, c) = t; }
            const double piv = M20(k, k);
            for (int c = k + 1; c < 20; c++) M20(k, c) = M20(k, c) / piv;
            M20(k, k) = 1.;
            for (int rr = 0; rr < 10; rr++) {
                if (rr == k) continue;
                const double f = M20(rr, k);
                for (int c = k + 1; c < 20; c++) M20(rr, c) = M20(rr, c) - f * M20(k, c);
                M20(rr, k) = 0.;
            }
        }
        // B(z) (rows k = e - z f, l = g - z h, m = i - z j) and its determinant, in registers; then both over the dead matrix
        {
            double bx[3][4], by[3][4], b1[3][5];
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const int hi = 4 + 2 * q, lo = 5 + 2 * q;
                bx[q][0] = -M20(lo, 10); bx[q][1] = M20(hi, 10) - M20(lo, 11); bx[q][2] = M20(hi, 11) - M20(lo, 12); bx[q][3] = M20(hi, 12);
                by[q][0] = -M20(lo, 13); by[q][1] = M20(hi, 13) - M20(lo, 14); by[q][2] = M20(hi, 14) - M20(lo, 15); by[q][3] = M20(hi, 15);
                b1[q][0] = -M20(lo, 16); b1[q][1] = M20(hi, 16) - M20(lo, 17); b1[q][2] = M20(hi, 17) - M20(lo, 18);
                b1[q][3] = M20(hi, 18) - M20(lo, 19); b1[q][4] = M20(hi, 19);
            }
            double u[8], v[8], w[7], w2[7], t0[11], t1[11], t2[11];
            e5_pmul<4, 5>(by[1], b1[2], u); e5_pmul<5, 4>(b1[1], by[2], v);
#pragma unroll
            for (int q = 0; q < 8; q++) u[q] = u[q] - v[q];
            e5_pmul<4, 8>(bx[0], u, t0);
            e5_pmul<4, 5>(bx[1], b1[2], u); e5_pmul<5, 4>(b1[1], bx[2], v);
#pragma unroll
            for (int q = 0; q < 8; q++) u[q] = u[q] - v[q];
            e5_pmul<4, 8>(by[0], u, t1);
            e5_pmul<4, 4>(bx[1], by[2], w); e5_pmul<4, 4>(by[1], bx[2], w2);
#pragma unroll
            for (int q = 0; q < 7; q++) w[q] = w[q] - w2[q];
            e5_pmul<5, 7>(b1[0], w, t2);
#pragma unroll
            for (int q = 0; q < 3; q++) {
#pragma unroll
                for (int i = 0; i < 4; i++) { BZ(13 * q + i) = bx[q][i]; BZ(13 * q + 4 + i) = by[q][i]; }
#pragma unroll
                for (int i = 0; i < 5; i++) BZ(13 * q + 8 + i) = b1[q][i];
            }
#pragma unroll
            for (int q = 0; q < 11; q++) PC(q) = (t0[q] - t1[q]) + t2[q];
        }
        // ---- 4: the real roots, ascending: Sturm counts inside the Cauchy bound, bisection, Newton ----
        int n_roots = 0;
        {
            const double c0 = PC(0);
            bool fin = c0 != 0.;
            double B = 0.;
            for (int k = 0; k < 11; k++) fin = fin && e5_finite(PC(k));
            if (fin) {
                for (int k = 1; k < 11; k++) { const double q = fabs(PC(k) / c0); B = q > B ? q : B; }
                B = 1. + B;
                fin = e5_finite(B);
            }
            if (fin) {
                for (int i = 0; i < 11; i++) ST(0, i) = PC(i);
                for (int i = 0; i < 10; i++) ST(1, i) = (double)(10 - i) * PC(i);
                for (int k = 1; k < 10; k++) {
                    const int da = 11 - k, db = 10 - k;
                    const double b0 = ST(k, 0), q1 = ST(k - 1, 0) / b0;
                    for (int i = 0; i < da; i++) ST(k + 1, i) = i < db ? ST(k - 1, i + 1) - q1 * ST(k, i + 1) : ST(k - 1, i + 1);
                    const double q0 = ST(k + 1, 0) / b0;
                    for (int i = 0; i < db; i++) ST(k + 1, i) = -(ST(k + 1, i + 1) - q0 * ST(k, i + 1));
                }
                const int v_lo = e5_sign_changes(sm, lane, -B);
                int total = v_lo - e5_sign_changes(sm, lane, B);
                total = total < 0 ? 0 : (total > 10 ? 10 : total);
                for (int j = 0; j < total; j++) {
                    double lo = -B, hi = B;
                    int n_lo = 0, n_hi = total;
                    for (int q = 0; q < E5_ISOLATE; q++) {
                        if (n_lo == j && n_hi == j + 1) break;
                        const double mid = (lo + hi) / 2.;
                        const int n_mid = v_lo - e5_sign_changes(sm, lane, mid);
                        if (n_mid >= j + 1) { hi = mid; n_hi = n_mid; } else { lo = mid; n_lo = n_mid; }
                    }
                    double v, d;
                    e5_horner(sm, lane, lo, v, d);
                    const bool pos_lo = v > 0.;
                    for (int q = 0; q < E5_REFINE; q++) {
                        const double mid = (lo + hi) / 2.;
                        e5_horner(sm, lane, mid, v, d);
                        if ((v > 0.) == pos_lo) lo = mid; else hi = mid;
                    }
                    double x = (lo + hi) / 2.;
                    for (int q = 0; q < E5_NEWTON; q++) {
                        e5_horner(sm, lane, x, v, d);
                        const double xn = x - v / d;
                        if (e5_finite(xn) && lo <= xn && xn <= hi) x = xn;
                    }
                    RT(j) = x;
                }
                n_roots = total;
            }
        }
        // ---- 5-7: per root x, y and E; Horn's four (R, t); the smallest sum of distances over the eight matches ----
        double best_s = 0.;
        for (int j = 0; j < n_roots; j++) {
            const double z = RT(j);
            double b[3][3];
#pragma unroll
            for (int q = 0; q < 3; q++) {
                double vx = BZ(13 * q), vy = BZ(13 * q + 4), v1 = BZ(13 * q + 8);
#pragma unroll
                for (int i = 1; i < 4; i++) { vx = vx * z + BZ(13 * q + i); vy = vy * z + BZ(13 * q + 4 + i); }
#pragma unroll
                for (int i = 1; i < 5; i++) v1 = v1 * z + BZ(13 * q + 8 + i);
                b[q][0] = vx; b[q][1] = vy; b[q][2] = v1;
            }
            const double d01 = b[0][0] * b[1][1] - b[0][1] * b[1][0], d02 = b[0][0] * b[2][1] - b[0][1] * b[2][0];
            const double d12 = b[1][0] * b[2][1] - b[1][1] * b[2][0];
            double bd = -1., det = 0., p0 = 0., p1 = 0., p2 = 0., q0 = 0., q1 = 0., q2 = 0.;
            bool any = false;
            if (fabs(d01) > bd) { bd = fabs(d01); det = d01; p0 = b[0][0]; p1 = b[0][1]; p2 = b[0][2]; q0 = b[1][0]; q1 = b[1][1]; q2 = b[1][2]; any = true; }
            if (fabs(d02) > bd) { bd = fabs(d02); det = d02; p0 = b[0][0]; p1 = b[0][1]; p2 = b[0][2]; q0 = b[2][0]; q1 = b[2][1]; q2 = b[2][2]; any = true; }
            if (fabs(d12) > bd) { bd = fabs(d12); det = d12; p0 = b[1][0]; p1 = b[1][1]; p2 = b[1][2]; q0 = b[2][0]; q1 = b[2][1]; q2 = b[2][2]; any = true; }
            if (!any) continue;
            const double x = (q2 * p1 - p2 * q1) / det, y = (p2 * q0 - q2 * p0) / det;
            double E[9];
            bool fin = true;
#pragma unroll
            for (int q = 0; q < 9; q++) {
                E[q] = ((x * NV(0, q) + y * NV(1, q)) + z * NV(2, q)) + NV(3, q);
                fin = fin && e5_finite(E[q]);
            }
            if (!fin) continue;
            // Horn: E scaled to tr(E E^T) = 2, b b^T = I - E E^T, R = Cof(E) -+ [b]x E
            double tr = 0.;
#pragma unroll
            for (int q = 0; q < 9; q++) tr = tr + E[q] * E[q];
            const double sc = sqrt(tr / 2.);
#pragma unroll
            for (int q = 0; q < 9; q++) E[q] = E[q] / sc;
            const E5V e0{E[0], E[1], E[2]}, e1{E[3], E[4], E[5]}, e2{E[6], E[7], E[8]};
            const double g00 = 1. - e5_dot(e0, e0), g11 = 1. - e5_dot(e1, e1), g22 = 1. - e5_dot(e2, e2);
            const double g01 = 0. - e5_dot(e0, e1), g02 = 0. - e5_dot(e0, e2), g12 = 0. - e5_dot(e1, e2);
            E5V gr3{g00, g01, g02};
            double gd = g00;
            if (g11 > gd) { gr3 = E5V{g01, g11, g12}; gd = g11; }
            if (g22 > gd) { gr3 = E5V{g02, g12, g22}; gd = g22; }
            const double sg = sqrt(gd);
            const E5V bb{gr3.x / sg, gr3.y / sg, gr3.z / sg};
            const E5V k0 = e5_cross(e1, e2), k1 = e5_cross(e2, e0), k2 = e5_cross(e0, e1);
            const E5V x0 = e5_cross(bb, E5V{E[0], E[3], E[6]}), x1 = e5_cross(bb, E5V{E[1], E[4], E[7]}), x2 = e5_cross(bb, E5V{E[2], E[5], E[8]});
            const double cof[9] = {k0.x, k0.y, k0.z, k1.x, k1.y, k1.z, k2.x, k2.y, k2.z};
            const double bE[9] = {x0.x, x1.x, x2.x, x0.y, x1.y, x2.y, x0.z, x1.z, x2.z};
            for (int c = 0; c < 4; c++) {                          // (b, E), (b, -E), (-b, E), (-b, -E)
                E5Model m;
                const bool minus = c == 0 || c == 3;
                fin = true;
#pragma unroll
                for (int q = 0; q < 9; q++) {
                    m.R[q] = minus ? cof[q] - bE[q] : cof[q] + bE[q];
                    fin = fin && e5_finite(m.R[q]);
                }
                m.t = c < 2 ? bb : E5V{-bb.x, -bb.y, -bb.z};
                fin = fin && e5_finite(m.t.x) && e5_finite(m.t.y) && e5_finite(m.t.z);
                if (!fin) continue;
                double s = 0.;
#pragma unroll
                for (int q = 0; q < 8; q++) s = s + e5_dist(m, e5_load(bv1, idx[q]), e5_load(bv2, idx[q]));
                if (!e5_finite(s)) continue;
                if (!have || s < best_s) { best = m; best_s = s; have = true; }
            }
        }
    }
    double *o = a.models + 12 * gr;
#pragma unroll
    for (int q = 0; q < 9; q++) o[q] = have ? best.R[q] : 0.;
    o[9] = have ? best.t.x : 0.; o[10] = have ? best.t.y : 0.; o[11] = have ? best.t.z : 0.;
    a.valid[gr] = have ? 1 : 0;
}

__device__ __forceinline__ E5Model e5_load_model(const double *o)
{
    E5Model m;
#pragma unroll
    for (int q = 0; q < 9; q++) m.R[q] = o[q];
    m.t = E5V{o[9], o[10], o[11]};
    return m;
}

__global__ __launch_bounds__(64) void k_e5_score(E5Args a)
{
    const E5Item it = a.items[blockIdx.y];
    const int r = blockIdx.x, lane = threadIdx.x;
    if (r >= it.S) return;
    const size_t gr = (size_t)it.row0 + (size_t)r;
    if (!a.valid[gr]) {
        if (lane == 0) a.score[gr] = 0.0;
        return;
    }
    const E5Model m = e5_load_model(a.models + 12 * gr);
    const double *bv1 = a.bv1 + 3 * (size_t)it.pt0, *bv2 = a.bv2 + 3 * (size_t)it.pt0;
    const int n = it.n;
    int cnt = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const bool in = i < n && e5_dist(m, e5_load(bv1, i), e5_load(bv2, i)) < a.threshold;
        cnt += __popcll(__ballot(in));
    }
    if (lane == 0) a.score[gr] = (double)cnt;
}

__global__ __launch_bounds__(64) void k_e5_pick(E5Args a)
{
    const E5Item it = a.items[blockIdx.x];
    const int lane = threadIdx.x, n = it.n;
    E5Out &out = a.out[blockIdx.x];
    int best_row = -1, iterations = 0, consumed = 0, status = 0;
    double best_score = 0.0;
    if (n < 8) {
        status = OV2_EPI_TOO_FEW_POINTS;
    } else {
        if (lane == 0) {
            const uint8_t *valid = a.valid + it.row0;
            const double *score = a.score + it.row0;
            int r = 0;
            double best = -1.0, k = 1.0;
            const double lp = log(1.0 - a.probability);
            while ((double)iterations < k && r < it.S) {
                const int cur = r++;
                if (!valid[cur]) continue;
                if (score[cur] > best) {
                    best = score[cur]; best_row = cur;
                    const double w = best / (double)n, w2 = w * w, w4 = w2 * w2;
                    double q = 1.0 - w4 * w4;
                    q = q > DBL_EPSILON ? q : DBL_EPSILON;
                    q = q < 1.0 - DBL_EPSILON ? q : 1.0 - DBL_EPSILON;
                    k = lp / log(q);
                }
                iterations++;
                if (iterations > a.max_iterations) break;
            }
            best_score = best_row >= 0 ? best : 0.0;
            consumed = r;
        }
        best_row = __shfl(best_row, 0);
        if (best_row < 0) status = OV2_EPI_NO_MODEL | OV2_EPI_FEW_INLIERS;
    }
    int n_out = 0, n_in = 0;
    E5Model m{};
    if (best_row >= 0) {
        m = e5_load_model(a.models + 12 * ((size_t)it.row0 + (size_t)best_row));
        const double *bv1 = a.bv1 + 3 * (size_t)it.pt0, *bv2 = a.bv2 + 3 * (size_t)it.pt0;
        int *ol = a.outliers + it.pt0;
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            const bool live = i < n;
            const bool in = live && e5_dist(m, e5_load(bv1, i), e5_load(bv2, i)) < a.threshold;
            const unsigned long long mo = __ballot(live && !in);
            if (live && !in) ol[n_out + __popcll(mo & ((1ull << lane) - 1ull))] = i;
            n_out += __popcll(mo);
            n_in += __popcll(__ballot(in));
        }
        if (n_in < E5_MIN_INLIERS) status |= OV2_EPI_FEW_INLIERS;
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 9; q++) out.model[q] = m.R[q];
        out.model[9] = m.t.x; out.model[10] = m.t.y; out.model[11] = m.t.z;
        out.score = best_score; out.best_row = best_row; out.iterations = iterations; out.rows_consumed = consumed;
        out.status = status; out.n_inliers = n_in; out.n_outliers = n_out;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
int e5_enqueue(hipStream_t s, const E5Args &a, int n_items, int s_max)
{
    if (n_items <= 0) return OV2_OK;
    if (s_max > 0) {
        hipLaunchKernelGGL(k_e5_solve, dim3((s_max + E5_LANES - 1) / E5_LANES, n_items), dim3(E5_LANES), 0, s, a);
        OV2_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_e5_score, dim3(s_max, n_items), dim3(64), 0, s, a);
        OV2_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_e5_pick, dim3(n_items), dim3(64), 0, s, a);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

int ov2_epipolar_draw_samples(unsigned long long seed, int n, int rows, int *out)
{
    OV2_REQUIRE(n >= 8, OV2_EINVAL, "ov2_epipolar_draw_samples: eight distinct indices need n >= 8");
    OV2_REQUIRE(rows >= 0, OV2_EINVAL, "ov2_epipolar_draw_samples: rows < 0");
    OV2_REQUIRE(rows == 0 || out, OV2_EINVAL, "ov2_epipolar_draw_samples: NULL out");
    unsigned long long j = 0;
    for (int r = 0; r < rows; r++)
        for (int k = 0; k < 8;) {
            const int v = (int)(e5_splitmix64(seed, j++) % (unsigned long long)n);
            bool dup = false;
            for (int q = 0; q < k; q++) dup = dup || out[8 * r + q] == v;
            if (!dup) out[8 * r + k++] = v;
        }
    return OV2_OK;
}

int ov2_epipolar_ransac_batch(ov2_ctx *ctx, const ov2_epipolar_params *params, int n_items, const ov2_epipolar_problem *problems,
                              ov2_epipolar_result *results)
{
    // the inputs first, the context last: a malformed input is reported without a device
    OV2_REQUIRE(params, OV2_EINVAL, "NULL params");
    OV2_REQUIRE(n_items >= 0, OV2_EINVAL, "n_items < 0");
    OV2_REQUIRE(n_items == 0 || (problems && results), OV2_EINVAL, "NULL problem / result array");
    OV2_REQUIRE(n_items <= 65535, OV2_EINVAL, "more than 65535 problems in one call");
    OV2_REQUIRE(!params->boptimize, OV2_EINVAL, "boptimize is not provided: OpenGV's non-linear refinement has no device form");
    OV2_REQUIRE(params->max_iterations >= 0, OV2_EINVAL, "max_iterations < 0");
    OV2_REQUIRE(std::isfinite(params->threshold) && params->threshold > 0.0, OV2_EINVAL, "threshold <= 0 or not finite");
    OV2_REQUIRE(params->probability > 0.0 && params->probability < 1.0, OV2_EINVAL, "probability outside (0, 1)");
    size_t NP = 0, NR = 0;
    int s_max = 0;
    bool trace = false, trace_model = false;
    for (int b = 0; b < n_items; b++) {
        const ov2_epipolar_problem &p = problems[b];
        const ov2_epipolar_result &r = results[b];
        OV2_REQUIRE(p.n >= 0 && p.n_rows >= 0, OV2_EINVAL, "negative count (n / n_rows)");
        OV2_REQUIRE(p.n <= E5_MAX_POINTS, OV2_EINVAL, "capacity: more than 2048 points in one problem");
        OV2_REQUIRE(p.n_rows <= E5_MAX_ROWS, OV2_EINVAL, "capacity: more than 4096 sample rows in one problem");
        OV2_REQUIRE(p.n == 0 || (p.bv1 && p.bv2), OV2_EINVAL, "NULL bv1 / bv2");
        OV2_REQUIRE(p.n_rows == 0 || p.samples, OV2_EINVAL, "NULL samples");
        OV2_REQUIRE(p.n == 0 || r.outliers, OV2_EINVAL, "NULL result buffer (outliers)");
        for (size_t i = 0; i < 3 * (size_t)p.n; i++)
            OV2_REQUIRE(std::isfinite(p.bv1[i]) && std::isfinite(p.bv2[i]), OV2_EINVAL, "bv1 / bv2 not finite");
        trace = trace || r.trace_valid || r.trace_score || r.trace_model;
        trace_model = trace_model || r.trace_model;
        NP += (size_t)p.n; NR += (size_t)p.n_rows;
        s_max = p.n_rows > s_max ? p.n_rows : s_max;
    }
    OV2_REQUIRE(NP <= 0x7fffffff && NR <= 0x7fffffff, OV2_EINVAL, "capacity: more than 2^31 - 1 points or rows in one call");
    OV2_REQUIRE(ctx, OV2_EINVAL, "NULL context");
    if (n_items == 0) return OV2_OK;

    // staging: [items 16 B][bv1 24][bv2 24][samples 32] up, [out 128][outliers 4][valid 1][score 8][models 96] down (valid and score
    // only for a trace, models only for a model trace); every section 16-byte aligned
    const size_t B = (size_t)n_items;
    StageCursor c(16);
    const size_t o_it = c.take(sizeof(E5Item) * B), o_b1 = c.take(24 * NP), o_b2 = c.take(24 * NP), o_sm = c.take(32 * NR);
    const size_t o_out = c.take(sizeof(E5Out) * B), o_ol = c.take(4 * NP), o_va = c.take(NR), o_sc = c.take(8 * NR), o_md = c.take(96 * NR);
    const size_t total = c.off;
    const size_t down_end = NR == 0 ? o_va : (trace_model ? total : (trace ? o_md : o_va));
    Stage st;
    int rc = st.open(ctx, total, down_end);  if (rc) return rc;
    uint8_t *hs = st.h, *ds = st.d;
    size_t pt0 = 0, row0 = 0;
    for (int b = 0; b < n_items; b++) {
        const ov2_epipolar_problem &p = problems[b];
        const E5Item it{p.n, p.n_rows, (int)pt0, (int)row0};
        memcpy(hs + o_it + sizeof(E5Item) * b, &it, sizeof(E5Item));
        if (p.n) {
            memcpy(hs + o_b1 + 24 * pt0, p.bv1, 24 * (size_t)p.n);
            memcpy(hs + o_b2 + 24 * pt0, p.bv2, 24 * (size_t)p.n);
        }
        if (p.n_rows) memcpy(hs + o_sm + 32 * row0, p.samples, 32 * (size_t)p.n_rows);
        pt0 += (size_t)p.n; row0 += (size_t)p.n_rows;
    }
    rc = st.upload(0, o_out);  if (rc) return rc;
    E5Args a;
    a.items = (const E5Item *)(ds + o_it); a.bv1 = (const double *)(ds + o_b1); a.bv2 = (const double *)(ds + o_b2);
    a.samples = (const int4 *)(ds + o_sm); a.models = (double *)(ds + o_md); a.valid = ds + o_va; a.score = (double *)(ds + o_sc);
    a.out = (E5Out *)(ds + o_out); a.outliers = (int *)(ds + o_ol);
    a.max_iterations = params->max_iterations; a.threshold = params->threshold; a.probability = params->probability;
    rc = e5_enqueue(ctx->stream, a, n_items, s_max);
    if (rc) return rc;
    rc = st.download(o_out, down_end, o_out);  if (rc) return rc;
    rc = st.sync();  if (rc) return rc;
    pt0 = row0 = 0;
    for (int b = 0; b < n_items; b++) {
        const ov2_epipolar_problem &p = problems[b];
        ov2_epipolar_result &r = results[b];
        E5Out o;
        memcpy(&o, hs + o_out + sizeof(E5Out) * b, sizeof(E5Out));
        memcpy(r.model, o.model, sizeof(o.model));
        r.score = o.score; r.best_row = o.best_row; r.iterations = o.iterations; r.rows_consumed = o.rows_consumed;
        r.status = o.status; r.n_inliers = o.n_inliers; r.n_outliers = o.n_outliers;
        if (o.n_outliers > 0) memcpy(r.outliers, hs + o_ol + 4 * pt0, 4 * (size_t)o.n_outliers);
        if (p.n_rows) {
            if (r.trace_valid) memcpy(r.trace_valid, hs + o_va + row0, (size_t)p.n_rows);
            if (r.trace_score) memcpy(r.trace_score, hs + o_sc + 8 * row0, 8 * (size_t)p.n_rows);
            if (r.trace_model) memcpy(r.trace_model, hs + o_md + 96 * row0, 96 * (size_t)p.n_rows);
        }
        pt0 += (size_t)p.n; row0 += (size_t)p.n_rows;
    }
    return OV2_OK;
}

int ov2_epipolar_ransac(ov2_ctx *ctx, const ov2_epipolar_params *params, const ov2_epipolar_problem *problem, ov2_epipolar_result *result)
{
    OV2_REQUIRE(problem && result, OV2_EINVAL, "NULL problem / result");
    return ov2_epipolar_ransac_batch(ctx, params, 1, problem, result);
}
