// p3p.hip -- absolute pose from 2D-3D matches for gfx950 (the reference's MultiViewGeometry::p3pRansac with USE_OPENGV,
// src/multi_view_geometry.cpp:144-343: AbsolutePoseSacProblem::KNEIP under sac::Lmeds or sac::Ransac).  OpenGV is not available to
// this project: the solver and the two loops are restated (tests/p3p_ref.py is the same specification in numpy), nothing is pinned
// against an OpenGV binary.  The sample table is an INPUT, so a call is a deterministic function of its arguments:
//   k_p3p_solve   ONE LANE PER (problem, row): Kneip's P3P on the row's first three indices (Ferrari's closed form for the quartic
//                 polished by complex Newton steps; each root's real part, two real Newton steps, accepted by residual; a pose must
//                 reproduce its three bearings to be a solution), the fourth index picks among the solutions.
//                 Writes the 3x4 model and a valid flag per row.
//   k_p3p_score   ONE WAVEFRONT PER (problem, row), lanes striding over the points.  RANSAC: inliers counted with ballots.  LMedS:
//                 the exact order statistics d[mid-1], d[mid] by bisection on the distances' 64-bit patterns (distances are >= 0,
//                 so the patterns order like unsigned integers) with wavefront counts; the distances stay in registers up to
//                 P3_REG * 64 points and in LDS above.
//   k_p3p_pick    ONE WAVEFRONT PER PROBLEM: lane 0 replays the sequential loop over the per-row scores (skipped rows do not
//                 count, strict comparisons, RANSAC's adaptive iteration bound), then all lanes classify the points against the
//                 winning model with the same p3_dist and write the ascending outlier list by ballot-prefix compaction.
// No atomics, no result that depends on scheduling.  Every pointer and size is validated on the host before any device work; the
// kernels check every sample index against the problem's point count before they read through it.
#include "common.hpp"
#include "p3p_dev.hpp"                 // P3Item, P3Out and the host steps (plan, stage, enqueue) that pnp.hip chains as well
#include <cmath>
#include <cfloat>

#pragma clang fp contract(off)

#define P3_MAX_POINTS 2048
#define P3_MAX_ROWS 4096
#define P3_BEARING_TOL 1e-12           // tests/p3p_ref.py, BEARING_TOL
#define P3_REG 8                       // distances per lane kept in registers: up to 512 points

struct P3V { double x, y, z; };
__device__ __forceinline__ P3V p3_sub(P3V a, P3V b) { return P3V{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ P3V p3_cross(P3V a, P3V b) { return P3V{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double p3_dot(P3V a, P3V b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ P3V p3_div(P3V a, double s) { return P3V{a.x / s, a.y / s, a.z / s}; }
__device__ __forceinline__ P3V p3_load(const double *p, size_t i) { return P3V{p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
struct P3M { P3V r0, r1, r2; };        // rows
__device__ __forceinline__ P3V p3_mul(const P3M &m, P3V v) { return P3V{p3_dot(m.r0, v), p3_dot(m.r1, v), p3_dot(m.r2, v)}; }
__device__ __forceinline__ P3V p3_mulT(const P3M &m, P3V v)
{
    return P3V{(m.r0.x * v.x + m.r1.x * v.y) + m.r2.x * v.z, (m.r0.y * v.x + m.r1.y * v.y) + m.r2.y * v.z, (m.r0.z * v.x + m.r1.z * v.y) + m.r2.z * v.z};
}
struct P3Model { P3M R; P3V C; };      // Rwc (row-major), camera centre

// d = max(0, 1 - bv . v / |v|), v = R^T (X - C); NaN (X == C) counts as 0.  The ONE distance of the score and of the pick.
__device__ __forceinline__ double p3_dist(const P3Model &m, P3V bv, P3V X)
{
    P3V v = p3_mulT(m.R, p3_sub(X, m.C));
    v = p3_div(v, sqrt(p3_dot(v, v)));
    const double d = 1.0 - p3_dot(bv, v);
    return d > 0.0 ? d : 0.0;
}

struct P3Args {
    const P3Item *items; const double *bv; const double *X; const int4 *samples;
    double *models; uint8_t *valid; double *score;
    P3Out *out; int *outliers;
    int mode, max_iterations; double threshold, probability;
};

// p(x), p'(x) and sum |c_k| |x|^k by Horner, as tests/p3p_ref.py
__device__ __forceinline__ void p3_poly(double c0, double c1, double c2, double c3, double c4, double x, double &v, double &d, double &m)
{
    const double ax = fabs(x);
    v = c0; d = 0.0; m = fabs(c0);
    d = d * x + v; v = v * x + c1; m = m * ax + fabs(c1);
    d = d * x + v; v = v * x + c2; m = m * ax + fabs(c2);
    d = d * x + v; v = v * x + c3; m = m * ax + fabs(c3);
    d = d * x + v; v = v * x + c4; m = m * ax + fabs(c4);
}

// The four roots (real and imaginary parts) of x^4 + a3 x^3 + a2 x^2 + a1 x + a0 (Ferrari: one real root of the resolvent cubic, two
// quadratics).  Accuracy is not the point here: the caller polishes every root by complex Newton steps.
__device__ __forceinline__ void p3_quartic(double a3, double a2, double a1, double a0, double x[4], double y[4])
{
    const double s4 = a3 * 0.25, a3_2 = a3 * a3;
    const double p = a2 - 0.375 * a3_2;
    const double q = a1 - 0.5 * a2 * a3 + 0.125 * a3_2 * a3;
    const double r = a0 - 0.25 * a1 * a3 + 0.0625 * a2 * a3_2 - (3.0 / 256.0) * a3_2 * a3_2;
    // resolvent m^3 + p m^2 + (p^2 / 4 - r) m - q^2 / 8 = 0: its largest real root is >= 0
    const double A = p, B = 0.25 * p * p - r, Cc = -0.125 * q * q;
    const double P = B - A * A / 3.0, Q = 2.0 * A * A * A / 27.0 - A * B / 3.0 + Cc;
    const double D = 0.25 * Q * Q + P * P * P / 27.0;
    double u;
    if (D > 0.0) {
        const double sD = sqrt(D);
        const double u1 = cbrt(Q > 0.0 ? -0.5 * Q - sD : -0.5 * Q + sD);
        u = u1 != 0.0 ? u1 - P / (3.0 * u1) : 0.0;
    } else if (P < 0.0) {
        const double sp = sqrt(-P / 3.0);
        double ca = 1.5 * Q / (P * sp);
        ca = ca > 1.0 ? 1.0 : (ca < -1.0 ? -1.0 : ca);
        u = 2.0 * sp * cos(acos(ca) / 3.0);
    } else {
        u = 0.0;
    }
    double m = u - A / 3.0;
#pragma unroll
    for (int k = 0; k < 2; k++) {                                  // two Newton steps on the cubic
        const double g = ((m + A) * m + B) * m + Cc, dg = (3.0 * m + 2.0 * A) * m + B;
        const double mn = m - g / dg;
        m = (dg != 0.0 && mn == mn) ? mn : m;
    }
    if (m > 0.0) {
        const double s = sqrt(2.0 * m), h = 0.5 * p + m, t = q / (2.0 * s);
        // y^2 - s y + (h + t) = 0 and y^2 + s y + (h - t) = 0
        const double d1 = 0.25 * s * s - (h + t), d2 = 0.25 * s * s - (h - t);
        const double e1 = d1 > 0.0 ? sqrt(d1) : 0.0, e2 = d2 > 0.0 ? sqrt(d2) : 0.0;
        const double i1 = d1 < 0.0 ? sqrt(-d1) : 0.0, i2 = d2 < 0.0 ? sqrt(-d2) : 0.0;
        x[0] = 0.5 * s + e1; x[1] = 0.5 * s - e1; x[2] = -0.5 * s + e2; x[3] = -0.5 * s - e2;
        y[0] = i1; y[1] = -i1; y[2] = i2; y[3] = -i2;
    } else {                                                       // q == 0: biquadratic in y^2
        const double disc = p * p - 4.0 * r;
        if (disc >= 0.0) {
            const double sd = sqrt(disc), z1 = 0.5 * (-p + sd), z2 = 0.5 * (-p - sd);
            const double y1 = z1 > 0.0 ? sqrt(z1) : 0.0, y2 = z2 > 0.0 ? sqrt(z2) : 0.0;
            const double j1 = z1 < 0.0 ? sqrt(-z1) : 0.0, j2 = z2 < 0.0 ? sqrt(-z2) : 0.0;
            x[0] = y1; x[1] = -y1; x[2] = y2; x[3] = -y2;
            y[0] = j1; y[1] = -j1; y[2] = j2; y[3] = -j2;
        } else {                                                   // y^2 = (-p +- i sqrt(-disc)) / 2, of modulus sqrt(r)
            const double re = sqrt(0.5 * (sqrt(r) - 0.5 * p)), im = sqrt(0.5 * (sqrt(r) + 0.5 * p));
            x[0] = re; x[1] = -re; x[2] = re; x[3] = -re;
            y[0] = im; y[1] = -im; y[2] = -im; y[3] = im;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) x[k] -= s4;
}

__device__ __forceinline__ P3M p3_frame(P3V a, P3V b)              // rows a, e3 x a, e3 = a x b / |a x b|
{
    P3V e3 = p3_cross(a, b);
    e3 = p3_div(e3, sqrt(p3_dot(e3, e3)));
    return P3M{a, p3_cross(e3, a), e3};
}

__device__ __forceinline__ bool p3_finite(double v) { return fabs(v) <= DBL_MAX; }

__global__ __launch_bounds__(64) void k_p3p_solve(P3Args a)
{
    const P3Item it = a.items[blockIdx.y];
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= it.S) return;
    const size_t gr = (size_t)it.row0 + (size_t)r;
    const int4 s = a.samples[gr];
    const unsigned n = (unsigned)it.n;
    bool ok = (unsigned)s.x < n && (unsigned)s.y < n && (unsigned)s.z < n && (unsigned)s.w < n;
    ok = ok && s.x != s.y && s.x != s.z && s.x != s.w && s.y != s.z && s.y != s.w && s.z != s.w;
    P3Model best{};
    bool have = false;
    if (ok) {
        const double *bv = a.bv + 3 * (size_t)it.pt0, *X = a.X + 3 * (size_t)it.pt0;
        P3V f1 = p3_load(bv, s.x), f2 = p3_load(bv, s.y);
        const P3V f3 = p3_load(bv, s.z), f4 = p3_load(bv, s.w);
        P3V P1 = p3_load(X, s.x), P2 = p3_load(X, s.y);
        const P3V P3 = p3_load(X, s.z), P4 = p3_load(X, s.w);
        P3M T = p3_frame(f1, f2);
        P3V g3 = p3_mul(T, f3);
        if (g3.z > 0.0) {
            const P3V tf = f1; f1 = f2; f2 = tf;
            const P3V tp = P1; P1 = P2; P2 = tp;
            T = p3_frame(f1, f2);
            g3 = p3_mul(T, f3);
        }
        const P3V e12 = p3_sub(P2, P1), e13 = p3_sub(P3, P1);
        const double d12 = sqrt(p3_dot(e12, e12));
        const P3V n1 = p3_div(e12, d12);
        P3V n3 = p3_cross(n1, e13);
        n3 = p3_div(n3, sqrt(p3_dot(n3, n3)));
        const P3M N{n1, p3_cross(n3, n1), n3};
        const P3V pp = p3_mul(N, e13);
        const double p1 = pp.x, p2 = pp.y, phi1 = g3.x / g3.z, phi2 = g3.y / g3.z;
        const double cb = p3_dot(f1, f2);
        double b = sqrt(1.0 / (1.0 - cb * cb) - 1.0);
        if (cb < 0.0) b = -b;
        const double f1_2 = phi1 * phi1, f2_2 = phi2 * phi2;
        const double p1_2 = p1 * p1, p1_3 = p1_2 * p1, p1_4 = p1_3 * p1;
        const double p2_2 = p2 * p2, p2_3 = p2_2 * p2, p2_4 = p2_3 * p2;
        const double d_2 = d12 * d12, b_2 = b * b;
        const double c0 = -f2_2 * p2_4 - p2_4 * f1_2 - p2_4;
        const double c1 = 2.0 * p2_3 * d12 * b + 2.0 * f2_2 * p2_3 * d12 * b - 2.0 * phi2 * p2_3 * phi1 * d12;
        const double c2 = -f2_2 * p2_2 * p1_2 - f2_2 * p2_2 * d_2 * b_2 - f2_2 * p2_2 * d_2 + f2_2 * p2_4 + p2_4 * f1_2 + 2.0 * p1 * p2_2 * d12
                          + 2.0 * phi1 * phi2 * p1 * p2_2 * d12 * b - p2_2 * p1_2 * f1_2 + 2.0 * p1 * p2_2 * f2_2 * d12 - p2_2 * d_2 * b_2
                          - 2.0 * p1_2 * p2_2;
        const double c3 = 2.0 * p1_2 * p2 * d12 * b + 2.0 * phi2 * p2_3 * phi1 * d12 - 2.0 * f2_2 * p2_3 * d12 * b - 2.0 * p1 * p2 * d_2 * b;
        const double c4 = -2.0 * phi2 * p2_2 * phi1 * p1 * d12 * b + f2_2 * p2_2 * d_2 + 2.0 * p1_3 * d12 - p1_2 * d_2 + f2_2 * p2_2 * p1_2
                          - p1_4 - 2.0 * f2_2 * p2_2 * p1 * d12 + p2_2 * f1_2 * p1_2 + f2_2 * p2_2 * d_2 * b_2;
        double xs[4], ys[4];
        p3_quartic(c1 / c0, c2 / c0, c3 / c0, c4 / c0, xs, ys);
        double bestd = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            // The solver's part: complex Newton steps take the closed-form root, real or not, to a root of the quartic as written
            // (a real root stays real: its imaginary part is an exact 0 throughout).
            double zr = xs[k], zi = ys[k];
#pragma unroll
            for (int j = 0; j < 6; j++) {
                double vr = c0, vi = 0.0, dr = 0.0, di = 0.0, t;
                const double cc[4] = {c1, c2, c3, c4};
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    t = dr * zr - di * zi + vr; di = dr * zi + di * zr + vi; dr = t;
                    t = vr * zr - vi * zi + cc[q]; vi = vr * zi + vi * zr; vr = t;
                }
                const double dd = dr * dr + di * di;
                const double sr = (vr * dr + vi * di) / dd, si = (vi * dr - vr * di) / dd;
                if (dd > 0.0 && sr == sr && si == si) { zr -= sr; zi -= si; }
            }
            // The acceptance rule: the candidate's real part, two Newton steps, the residual
            double x = zr, v, d, m;
#pragma unroll
            for (int j = 0; j < 2; j++) {
                p3_poly(c0, c1, c2, c3, c4, x, v, d, m);
                x = x - v / d;
            }
            p3_poly(c0, c1, c2, c3, c4, x, v, d, m);
            if (!(fabs(x) <= 1.0 && fabs(v) <= 1e-9 * m)) continue;
            const double cot = (-phi1 * p1 / phi2 - x * p2 + d12 * b) / (-phi1 * x * p2 / phi2 + p1 - d12);
            const double ct = x, st = sqrt(1.0 - x * x);
            const double sa = sqrt(1.0 / (cot * cot + 1.0));
            double ca = sqrt(1.0 - sa * sa);
            if (cot < 0.0) ca = -ca;
            const double kk = d12 * (sa * b + ca);
            P3Model mdl;
            const P3V Cn = p3_mulT(N, P3V{ca * kk, ct * sa * kk, st * sa * kk});
            mdl.C = P3V{P1.x + Cn.x, P1.y + Cn.y, P1.z + Cn.z};
            // R = N^T Q^T T, Q = [-ca, -sa ct, -sa st; sa, -ca ct, -ca st; 0, -st, ct]: first W = Q^T T (rows), then N^T W
            const P3V q0{-ca, sa, 0.0}, q1{-sa * ct, -ca * ct, -st}, q2{-sa * st, -ca * st, ct};   // rows of Q^T
            const P3M W{p3_mulT(T, q0), p3_mulT(T, q1), p3_mulT(T, q2)};
            // (N^T W) row i = sum_j N[j][i] W[j]
            mdl.R.r0 = P3V{(N.r0.x * W.r0.x + N.r1.x * W.r1.x) + N.r2.x * W.r2.x, (N.r0.x * W.r0.y + N.r1.x * W.r1.y) + N.r2.x * W.r2.y,
                           (N.r0.x * W.r0.z + N.r1.x * W.r1.z) + N.r2.x * W.r2.z};
            mdl.R.r1 = P3V{(N.r0.y * W.r0.x + N.r1.y * W.r1.x) + N.r2.y * W.r2.x, (N.r0.y * W.r0.y + N.r1.y * W.r1.y) + N.r2.y * W.r2.y,
                           (N.r0.y * W.r0.z + N.r1.y * W.r1.z) + N.r2.y * W.r2.z};
            mdl.R.r2 = P3V{(N.r0.z * W.r0.x + N.r1.z * W.r1.x) + N.r2.z * W.r2.x, (N.r0.z * W.r0.y + N.r1.z * W.r1.y) + N.r2.z * W.r2.y,
                           (N.r0.z * W.r0.z + N.r1.z * W.r1.z) + N.r2.z * W.r2.z};
            // a solution reproduces its own three bearings: roots of the mirrored configuration (the elimination squares sin(theta)
            // away) and centres beyond point 1 or 2 (alpha + beta > pi) do not; a NaN fails
            if (!(p3_dist(mdl, f1, P1) <= P3_BEARING_TOL && p3_dist(mdl, f2, P2) <= P3_BEARING_TOL && p3_dist(mdl, f3, P3) <= P3_BEARING_TOL))
                continue;
            const double d4 = p3_dist(mdl, f4, P4);
            if (!have || d4 < bestd) { best = mdl; bestd = d4; have = true; }
        }
        if (have) {
            const P3M &R = best.R;
            have = p3_finite(R.r0.x) && p3_finite(R.r0.y) && p3_finite(R.r0.z) && p3_finite(R.r1.x) && p3_finite(R.r1.y) && p3_finite(R.r1.z) &&
                   p3_finite(R.r2.x) && p3_finite(R.r2.y) && p3_finite(R.r2.z) && p3_finite(best.C.x) && p3_finite(best.C.y) && p3_finite(best.C.z);
        }
    }
    double *o = a.models + 12 * gr;
    o[0] = best.R.r0.x; o[1] = best.R.r0.y; o[2] = best.R.r0.z;
    o[3] = best.R.r1.x; o[4] = best.R.r1.y; o[5] = best.R.r1.z;
    o[6] = best.R.r2.x; o[7] = best.R.r2.y; o[8] = best.R.r2.z;
    o[9] = best.C.x; o[10] = best.C.y; o[11] = best.C.z;
    a.valid[gr] = have ? 1 : 0;
}

__device__ __forceinline__ P3Model p3_load_model(const double *o)
{
    P3Model m;
    m.R.r0 = P3V{o[0], o[1], o[2]}; m.R.r1 = P3V{o[3], o[4], o[5]}; m.R.r2 = P3V{o[6], o[7], o[8]};
    m.C = P3V{o[9], o[10], o[11]};
    return m;
}

#define P3_PAD 0x7ff0000000000000ull    // the pattern of +inf: above every distance, never selected (k < n)

// The k-th smallest (0-based) of the wavefront's patterns, bit by bit from the top: at each bit the wavefront counts the values
// that share the prefix chosen so far and have the bit clear.  `below` receives the largest pattern strictly below the result
// when exactly k values lie below it, the result itself otherwise (equal values around the position).
template <bool LDS>
__device__ __forceinline__ unsigned long long p3_select(const unsigned long long (&reg)[P3_REG], const unsigned long long *sd, int per_lane,
                                                        int lane, int k, unsigned long long &below)
{
    unsigned long long res = 0;
    const int kk = k;
    for (int bit = 62; bit >= 0; bit--) {                          // bit 63 is the sign: clear
        const unsigned long long keep = ~((1ull << bit) - 1ull);   // this bit and everything above
        int c = 0;
        if (LDS) {
            for (int j = 0; j < per_lane; j++) c += __popcll(__ballot((sd[lane + 64 * j] & keep) == res));
        } else {
#pragma unroll
            for (int j = 0; j < P3_REG; j++) c += __popcll(__ballot((reg[j] & keep) == res));
        }
        if (k >= c) { k -= c; res |= 1ull << bit; }
    }
    int less = 0;
    unsigned long long mx = 0;
    if (LDS) {
        for (int j = 0; j < per_lane; j++) {
            const unsigned long long v = sd[lane + 64 * j];
            less += __popcll(__ballot(v < res));
            mx = (v < res && v > mx) ? v : mx;
        }
    } else {
#pragma unroll
        for (int j = 0; j < P3_REG; j++) {
            less += __popcll(__ballot(reg[j] < res));
            mx = (reg[j] < res && reg[j] > mx) ? reg[j] : mx;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long v = __shfl_xor(mx, o);
        mx = v > mx ? v : mx;
    }
    below = less == kk ? mx : res;
    return res;
}

__global__ __launch_bounds__(64) void k_p3p_score(P3Args a)
{
    extern __shared__ unsigned long long p3_sd[];                  // LMedS above P3_REG * 64 points: the distances' patterns
    const P3Item it = a.items[blockIdx.y];
    const int r = blockIdx.x, lane = threadIdx.x;
    if (r >= it.S) return;
    const size_t gr = (size_t)it.row0 + (size_t)r;
    if (!a.valid[gr]) {
        if (lane == 0) a.score[gr] = 0.0;
        return;
    }
    const P3Model m = p3_load_model(a.models + 12 * gr);
    const double *bv = a.bv + 3 * (size_t)it.pt0, *X = a.X + 3 * (size_t)it.pt0;
    const int n = it.n;
    double score;
    if (a.mode == OV2_P3P_RANSAC) {
        int cnt = 0;
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            const bool in = i < n && p3_dist(m, p3_load(bv, i), p3_load(X, i)) < a.threshold;
            cnt += __popcll(__ballot(in));
        }
        score = (double)cnt;
    } else {
        const int mid = n / 2;
        unsigned long long reg[P3_REG], lo, hi;
        if (n <= P3_REG * 64) {
#pragma unroll
            for (int j = 0; j < P3_REG; j++) {
                const int i = lane + 64 * j;
                reg[j] = i < n ? (unsigned long long)__double_as_longlong(p3_dist(m, p3_load(bv, i), p3_load(X, i))) : P3_PAD;
            }
            hi = p3_select<false>(reg, nullptr, 0, lane, mid, lo);
        } else {
            const int per_lane = (n + 63) / 64;
            for (int j = 0; j < per_lane; j++) {
                const int i = lane + 64 * j;
                p3_sd[i] = i < n ? (unsigned long long)__double_as_longlong(p3_dist(m, p3_load(bv, i), p3_load(X, i))) : P3_PAD;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < P3_REG; j++) reg[j] = P3_PAD;
            hi = p3_select<true>(reg, p3_sd, per_lane, lane, mid, lo);
        }
        const double dh = __longlong_as_double((long long)hi), dl = __longlong_as_double((long long)lo);
        score = (n & 1) ? sqrt(dh) : (sqrt(dl) + sqrt(dh)) / 2.0;
    }
    if (lane == 0) a.score[gr] = score;
}

__global__ __launch_bounds__(64) void k_p3p_pick(P3Args a)
{
    const P3Item it = a.items[blockIdx.x];
    const int lane = threadIdx.x, n = it.n;
    P3Out &out = a.out[blockIdx.x];
    int best_row = -1, iterations = 0, consumed = 0, status = 0;
    double best_score = 0.0;
    if (n < 4) {
        status = OV2_P3P_TOO_FEW_POINTS;
    } else {
        if (lane == 0) {
            const uint8_t *valid = a.valid + it.row0;
            const double *score = a.score + it.row0;
            int r = 0;
            if (a.mode == OV2_P3P_LMEDS) {
                double best = INFINITY;
                while (iterations < a.max_iterations && r < it.S) {
                    const int cur = r++;
                    if (!valid[cur]) continue;
                    if (score[cur] < best) { best = score[cur]; best_row = cur; }
                    iterations++;
                }
                best_score = best_row >= 0 ? best : 0.0;
            } else {
                double best = -1.0, k = 1.0;
                const double lp = log(1.0 - a.probability);
                while ((double)iterations < k && r < it.S) {
                    const int cur = r++;
                    if (!valid[cur]) continue;
                    if (score[cur] > best) {
                        best = score[cur]; best_row = cur;
                        const double w = best / (double)n;
                        double q = 1.0 - w * w * w * w;
                        q = q > DBL_EPSILON ? q : DBL_EPSILON;
                        q = q < 1.0 - DBL_EPSILON ? q : 1.0 - DBL_EPSILON;
                        k = lp / log(q);
                    }
                    iterations++;
                    if (iterations > a.max_iterations) break;
                }
                best_score = best_row >= 0 ? best : 0.0;
            }
            consumed = r;
        }
        best_row = __shfl(best_row, 0);
        if (best_row < 0) status = OV2_P3P_NO_MODEL | OV2_P3P_FEW_INLIERS;
    }
    int n_out = 0, n_in = 0;
    P3Model m{};
    if (best_row >= 0) {
        m = p3_load_model(a.models + 12 * ((size_t)it.row0 + (size_t)best_row));
        const double *bv = a.bv + 3 * (size_t)it.pt0, *X = a.X + 3 * (size_t)it.pt0;
        int *ol = a.outliers + it.pt0;
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            const bool live = i < n;
            const bool in = live && p3_dist(m, p3_load(bv, i), p3_load(X, i)) < a.threshold;
            const unsigned long long mo = __ballot(live && !in);
            if (live && !in) ol[n_out + __popcll(mo & ((1ull << lane) - 1ull))] = i;
            n_out += __popcll(mo);
            n_in += __popcll(__ballot(in));
        }
        if (n_in < 5) status |= OV2_P3P_FEW_INLIERS;
        // Sophus::isOrthogonal (rotation_matrix.hpp:25): |R R^T - I|_F < 1e-10
        const P3M &R = m.R;
        const double e00 = p3_dot(R.r0, R.r0) - 1.0, e11 = p3_dot(R.r1, R.r1) - 1.0, e22 = p3_dot(R.r2, R.r2) - 1.0;
        const double e01 = p3_dot(R.r0, R.r1), e02 = p3_dot(R.r0, R.r2), e12 = p3_dot(R.r1, R.r2);
        const double fro = sqrt(e00 * e00 + e11 * e11 + e22 * e22 + 2.0 * (e01 * e01 + e02 * e02 + e12 * e12));
        if (!(fro < 1e-10)) status |= OV2_P3P_NOT_ORTHOGONAL;
    }
    if (lane == 0) {
        out.model[0] = m.R.r0.x; out.model[1] = m.R.r0.y; out.model[2] = m.R.r0.z;
        out.model[3] = m.R.r1.x; out.model[4] = m.R.r1.y; out.model[5] = m.R.r1.z;
        out.model[6] = m.R.r2.x; out.model[7] = m.R.r2.y; out.model[8] = m.R.r2.z;
        out.model[9] = m.C.x; out.model[10] = m.C.y; out.model[11] = m.C.z;
        out.score = best_score; out.best_row = best_row; out.iterations = iterations; out.rows_consumed = consumed;
        out.status = status; out.n_inliers = n_in; out.n_outliers = n_out;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
static inline unsigned long long p3_splitmix64(unsigned long long seed, unsigned long long j)
{
    unsigned long long z = seed + (j + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int ov2_p3p_draw_samples(unsigned long long seed, int n, int rows, int *out)
{
    OV2_REQUIRE(n >= 4, OV2_EINVAL, "ov2_p3p_draw_samples: four distinct indices need n >= 4");
    OV2_REQUIRE(rows >= 0, OV2_EINVAL, "ov2_p3p_draw_samples: rows < 0");
    OV2_REQUIRE(rows == 0 || out, OV2_EINVAL, "ov2_p3p_draw_samples: NULL out");
    unsigned long long j = 0;
    for (int r = 0; r < rows; r++)
        for (int k = 0; k < 4;) {
            const int v = (int)(p3_splitmix64(seed, j++) % (unsigned long long)n);
            bool dup = false;
            for (int q = 0; q < k; q++) dup = dup || out[4 * r + q] == v;
            if (!dup) out[4 * r + k++] = v;
        }
    return OV2_OK;
}

static void p3p_plan_fill(P3Plan &pl, size_t B, size_t NP, size_t NR, int n_max, int s_max, bool trace)
{
    pl.B = B; pl.NP = NP; pl.NR = NR; pl.n_max = n_max; pl.s_max = s_max; pl.trace = trace;
    StageCursor c(16);
    pl.o_it = c.take(sizeof(P3Item) * B); pl.o_bv = c.take(24 * NP); pl.o_X = c.take(24 * NP); pl.o_sm = c.take(16 * NR);
    pl.o_out = c.take(sizeof(P3Out) * B); pl.o_ol = c.take(4 * NP); pl.o_va = c.take(NR); pl.o_sc = c.take(8 * NR);
    pl.o_md = c.take(96 * NR); pl.total = c.off;
}

int p3p_plan(const ov2_p3p_params *params, int n_items, const ov2_p3p_problem *problems, const ov2_p3p_result *results, P3Plan *plan)
{
    OV2_REQUIRE(params, OV2_EINVAL, "NULL params");
    OV2_REQUIRE(n_items >= 0, OV2_EINVAL, "n_items < 0");
    OV2_REQUIRE(n_items == 0 || problems, OV2_EINVAL, "NULL problem / result array");
    OV2_REQUIRE(n_items <= 65535, OV2_EINVAL, "more than 65535 problems in one call");
    OV2_REQUIRE(params->mode == OV2_P3P_LMEDS || params->mode == OV2_P3P_RANSAC, OV2_EINVAL, "mode is neither OV2_P3P_LMEDS nor OV2_P3P_RANSAC");
    OV2_REQUIRE(!params->boptimize, OV2_EINVAL, "boptimize is not provided: refine the pose with ov2_ba_solve (ov2::ceresPnP) afterwards");
    OV2_REQUIRE(params->max_iterations >= 0, OV2_EINVAL, "max_iterations < 0");
    OV2_REQUIRE(std::isfinite(params->threshold) && params->threshold > 0.0, OV2_EINVAL, "threshold <= 0 or not finite");
    OV2_REQUIRE(params->probability > 0.0 && params->probability < 1.0, OV2_EINVAL, "probability outside (0, 1)");
    size_t NP = 0, NR = 0;
    int n_max = 0, s_max = 0;
    bool trace = false;
    for (int b = 0; b < n_items; b++) {
        const ov2_p3p_problem &p = problems[b];
        OV2_REQUIRE(p.n >= 0 && p.n_rows >= 0, OV2_EINVAL, "negative count (n / n_rows)");
        OV2_REQUIRE(p.n <= P3_MAX_POINTS, OV2_EINVAL, "capacity: more than 2048 points in one problem");
        OV2_REQUIRE(p.n_rows <= P3_MAX_ROWS, OV2_EINVAL, "capacity: more than 4096 sample rows in one problem");
        OV2_REQUIRE(p.n == 0 || (p.bv && p.X), OV2_EINVAL, "NULL bv / X");
        OV2_REQUIRE(p.n_rows == 0 || p.samples, OV2_EINVAL, "NULL samples");
        if (results) {
            const ov2_p3p_result &r = results[b];
            OV2_REQUIRE(p.n == 0 || r.outliers, OV2_EINVAL, "NULL result buffer (outliers)");
            trace = trace || r.trace_valid || r.trace_score;
        }
        for (size_t i = 0; i < 3 * (size_t)p.n; i++)
            OV2_REQUIRE(std::isfinite(p.bv[i]) && std::isfinite(p.X[i]), OV2_EINVAL, "bv / X not finite");
        NP += (size_t)p.n; NR += (size_t)p.n_rows;
        n_max = p.n > n_max ? p.n : n_max; s_max = p.n_rows > s_max ? p.n_rows : s_max;
    }
    OV2_REQUIRE(NP <= 0x7fffffff && NR <= 0x7fffffff, OV2_EINVAL, "capacity: more than 2^31 - 1 points or rows in one call");
    p3p_plan_fill(*plan, (size_t)n_items, NP, NR, n_max, s_max, trace);
    return OV2_OK;
}

int p3p_plan_capacity(int n_items, int n_max, int n_rows, P3Plan *plan)
{
    OV2_REQUIRE(n_items >= 0 && n_items <= 65535, OV2_EINVAL, "more than 65535 problems in one call");
    OV2_REQUIRE(n_max >= 0 && n_max <= P3_MAX_POINTS, OV2_EINVAL, "capacity: more than 2048 points in one problem");
    OV2_REQUIRE(n_rows >= 0 && n_rows <= P3_MAX_ROWS, OV2_EINVAL, "capacity: more than 4096 sample rows in one problem");
    const size_t NP = (size_t)n_items * (size_t)n_max, NR = (size_t)n_items * (size_t)n_rows;
    OV2_REQUIRE(NP <= 0x7fffffff && NR <= 0x7fffffff, OV2_EINVAL, "capacity: more than 2^31 - 1 points or rows in one call");
    p3p_plan_fill(*plan, (size_t)n_items, NP, NR, n_max, n_rows, false);
    return OV2_OK;
}

void p3p_stage(const P3Plan &pl, const ov2_p3p_problem *problems, uint8_t *hs)
{
    size_t pt0 = 0, row0 = 0;
    for (size_t b = 0; b < pl.B; b++) {
        const ov2_p3p_problem &p = problems[b];
        const P3Item it{p.n, p.n_rows, (int)pt0, (int)row0};
        memcpy(hs + pl.o_it + sizeof(P3Item) * b, &it, sizeof(P3Item));
        if (p.n) {
            memcpy(hs + pl.o_bv + 24 * pt0, p.bv, 24 * (size_t)p.n);
            memcpy(hs + pl.o_X + 24 * pt0, p.X, 24 * (size_t)p.n);
        }
        if (p.n_rows) memcpy(hs + pl.o_sm + 16 * row0, p.samples, 16 * (size_t)p.n_rows);
        pt0 += (size_t)p.n; row0 += (size_t)p.n_rows;
    }
}

int p3p_enqueue(hipStream_t s, const ov2_p3p_params *params, const P3Plan &pl, uint8_t *ds)
{
    const int n_items = (int)pl.B;
    P3Args a;
    a.items = (const P3Item *)(ds + pl.o_it); a.bv = (const double *)(ds + pl.o_bv); a.X = (const double *)(ds + pl.o_X);
    a.samples = (const int4 *)(ds + pl.o_sm); a.models = (double *)(ds + pl.o_md); a.valid = ds + pl.o_va; a.score = (double *)(ds + pl.o_sc);
    a.out = (P3Out *)(ds + pl.o_out); a.outliers = (int *)(ds + pl.o_ol);
    a.mode = params->mode; a.max_iterations = params->max_iterations; a.threshold = params->threshold; a.probability = params->probability;
    if (pl.s_max > 0) {
        hipLaunchKernelGGL(k_p3p_solve, dim3((pl.s_max + 63) / 64, n_items), dim3(64), 0, s, a);
        OV2_HIP_CHECK(hipGetLastError());
        const size_t lds = (a.mode == OV2_P3P_LMEDS && pl.n_max > P3_REG * 64) ? 8 * 64 * (size_t)((pl.n_max + 63) / 64) : 0;
        hipLaunchKernelGGL(k_p3p_score, dim3(pl.s_max, n_items), dim3(64), lds, s, a);
        OV2_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_p3p_pick, dim3(n_items), dim3(64), 0, s, a);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

int ov2_p3p_ransac_batch(ov2_ctx *ctx, const ov2_p3p_params *params, int n_items, const ov2_p3p_problem *problems, ov2_p3p_result *results)
{
    // the inputs first, the context last: a malformed input is reported without a device
    OV2_REQUIRE(params, OV2_EINVAL, "NULL params");
    OV2_REQUIRE(n_items >= 0, OV2_EINVAL, "n_items < 0");
    OV2_REQUIRE(n_items == 0 || (problems && results), OV2_EINVAL, "NULL problem / result array");
    P3Plan pl;
    int rc = p3p_plan(params, n_items, problems, results, &pl);
    if (rc) return rc;
    OV2_REQUIRE(ctx, OV2_EINVAL, "NULL context");
    if (n_items == 0) return OV2_OK;

    Stage st;
    rc = st.open(ctx, pl.total, pl.o_md);  if (rc) return rc;     // (the models stay on the device: the host block ends where they begin)
    uint8_t *hs = st.h, *ds = st.d;
    p3p_stage(pl, problems, hs);
    rc = st.upload(0, pl.o_out);  if (rc) return rc;
    rc = p3p_enqueue(ctx->stream, params, pl, ds);
    if (rc) return rc;
    const size_t down_end = (pl.trace && pl.NR > 0) ? pl.o_md : pl.o_va;
    rc = st.download(pl.o_out, down_end, pl.o_out);  if (rc) return rc;
    rc = st.sync();  if (rc) return rc;
    size_t pt0 = 0, row0 = 0;
    for (int b = 0; b < n_items; b++) {
        const ov2_p3p_problem &p = problems[b];
        ov2_p3p_result &r = results[b];
        P3Out o;
        memcpy(&o, hs + pl.o_out + sizeof(P3Out) * b, sizeof(P3Out));
        memcpy(r.model, o.model, sizeof(o.model));
        r.score = o.score; r.best_row = o.best_row; r.iterations = o.iterations; r.rows_consumed = o.rows_consumed;
        r.status = o.status; r.n_inliers = o.n_inliers; r.n_outliers = o.n_outliers;
        if (o.n_outliers > 0) memcpy(r.outliers, hs + pl.o_ol + 4 * pt0, 4 * (size_t)o.n_outliers);
        if (p.n_rows) {
            if (r.trace_valid) memcpy(r.trace_valid, hs + pl.o_va + row0, (size_t)p.n_rows);
            if (r.trace_score) memcpy(r.trace_score, hs + pl.o_sc + 8 * row0, 8 * (size_t)p.n_rows);
        }
        pt0 += (size_t)p.n; row0 += (size_t)p.n_rows;
    }
    return OV2_OK;
}

int ov2_p3p_ransac(ov2_ctx *ctx, const ov2_p3p_params *params, const ov2_p3p_problem *problem, ov2_p3p_result *result)
{
    OV2_REQUIRE(problem && result, OV2_EINVAL, "NULL problem / result");
    return ov2_p3p_ransac_batch(ctx, params, 1, problem, result);
}
