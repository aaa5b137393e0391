"""The specification of the device 5-point essential-matrix search (csrc/fivept.hip, ov2_epipolar_ransac[_batch]) in numpy: the
reference's MultiViewGeometry::opengv5ptEssentialMatrix (src/multi_view_geometry.cpp:613-696), i.e. Nister's five-point solver under
OpenGV's sac::Ransac, replayed over a sample table that is an INPUT, so that the result is a function of the inputs alone.  OpenGV is
not available to this project: the solver and the loop are restated from the paper (Nister, PAMI 2004) and from the library's
published behaviour, and nothing here was compared with an OpenGV binary.  Where OpenGV's own choice is not known (whether the
disambiguation uses all eight sample matches or only the three extra ones, how a row without a model is treated, every rule at exact
equality) this file's choice is the definition.

The model is [R | t] with x1 = R x2 + t (the reference's Rwc, twc = Rkfc, tkfc), bv1^T [t]x R bv2 = 0, |t| = 1.

No np.linalg here: explicit eliminations and closed forms only, so that every function runs unchanged with F = np.float64 (the
specification) and F = np.longdouble (the same code in extended precision: the GPU test bounds the device by the distance between
the two, row by row, and rows on which the two DECIDE differently are marked fragile and compared on nothing)."""
import math

import numpy as np

TOO_FEW_POINTS, NO_MODEL, FEW_INLIERS = 1, 2, 4
MAX_POINTS, MAX_ROWS = 2048, 4096
SAMPLE = 8                             # indices per row: five for the solver, all eight for the disambiguation
MIN_INLIERS = 10                       # src/multi_view_geometry.cpp:665
ISOLATE_TRIPS, REFINE_TRIPS, NEWTON_STEPS = 40, 30, 3
_M64 = (1 << 64) - 1


# ---- sample table ----------------------------------------------------------------------------------------------------------------
def _splitmix64(seed, j):
    z = (seed + (j + 1) * 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def draw_samples(seed, n, rows):
    """rows x 8 int32: the stream of p3p_ref.draw_samples (draw j is splitmix64 of seed + (j + 1) * 0x9E3779B97F4A7C15, modulo n),
    eight distinct indices per row, a slot that repeats an earlier slot of its row is drawn again"""
    if n < SAMPLE or rows < 0:
        raise ValueError("draw_samples: n >= 8 and rows >= 0")
    out = np.zeros((rows, SAMPLE), np.int32)
    j = 0
    for r in range(rows):
        k = 0
        while k < SAMPLE:
            v = _splitmix64(seed & _M64, j) % n
            j += 1
            if v in out[r, :k]:
                continue
            out[r, k] = v
            k += 1
    return out


# ---- polynomials in (x, y, z) ------------------------------------------------------------------------------------------------------
# variables 0 = x, 1 = y, 2 = z, 3 = 1; a monomial is a sorted tuple of variables
_Q = [(i, j) for i in range(4) for j in range(i, 4)]                          # 10 monomials of degree <= 2
_C = [(i, j, k) for i in range(4) for j in range(i, 4) for k in range(j, 4)]  # 20 monomials of degree <= 3
_QI = {m: a for a, m in enumerate(_Q)}
_CI = {m: a for a, m in enumerate(_C)}
# Nister's order: x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1
NISTER = [(0, 0, 0), (1, 1, 1), (0, 0, 1), (0, 1, 1), (0, 0, 2), (0, 0, 3), (1, 1, 2), (1, 1, 3), (0, 1, 2), (0, 1, 3),
          (0, 2, 2), (0, 2, 3), (0, 3, 3), (1, 2, 2), (1, 2, 3), (1, 3, 3), (2, 2, 2), (2, 2, 3), (2, 3, 3), (3, 3, 3)]
_TO_NISTER = np.array([_CI[m] for m in NISTER])


def _mul11(a, b, F):
    """(4,) x (4,) linear forms -> (10,)"""
    q = np.zeros(10, F)
    for i in range(4):
        for j in range(4):
            q[_QI[(min(i, j), max(i, j))]] += a[i] * b[j]
    return q


def _mul21(q, l, F):
    """(10,) x (4,) -> (20,)"""
    c = np.zeros(20, F)
    for a, (i, j) in enumerate(_Q):
        for k in range(4):
            c[_CI[tuple(sorted((i, j, k)))]] += q[a] * l[k]
    return c


# ---- steps 1-2: the null space ---------------------------------------------------------------------------------------------------
def null_space(f1, f2, F=np.float64):
    """(4, 9): an orthonormal basis of the null space of the 5 x 9 matrix with rows kron(f1_i, f2_i): Gauss-Jordan with full
    pivoting (the first largest entry in row-major order wins), one basis vector per free column, modified Gram-Schmidt"""
    A = np.zeros((5, 9), F)
    for i in range(5):
        for a in range(3):
            A[i, 3 * a:3 * a + 3] = f1[i, a] * f2[i]
    perm = list(range(9))
    for k in range(5):
        pr, pc, big = k, k, F(-1)
        for r in range(k, 5):
            for c in range(k, 9):
                if abs(A[r, c]) > big:
                    pr, pc, big = r, c, abs(A[r, c])
        if pr != k:
            A[[k, pr]] = A[[pr, k]]
        if pc != k:
            A[:, [k, pc]] = A[:, [pc, k]]
            perm[k], perm[pc] = perm[pc], perm[k]
        A[k, k + 1:] = A[k, k + 1:] / A[k, k]
        A[k, k] = F(1)
        for r in range(5):
            if r != k:
                A[r, k + 1:] = A[r, k + 1:] - A[r, k] * A[k, k + 1:]
                A[r, k] = F(0)
    V = np.zeros((4, 9), F)
    for j in range(4):
        V[j, perm[5 + j]] = F(1)
        for i in range(5):
            V[j, perm[i]] = -A[i, 5 + j]
    for k in range(4):
        for j in range(k):
            d = F(0)
            for e in range(9):
                d = d + V[k, e] * V[j, e]
            V[k] = V[k] - d * V[j]
        s = F(0)
        for e in range(9):
            s = s + V[k, e] * V[k, e]
        V[k] = V[k] / np.sqrt(s)
    return V


# ---- step 3: the constraints ---------------------------------------------------------------------------------------------------------
def constraints(V, F=np.float64):
    """(10, 20) in Nister's monomial order: rows 0-8 the entries (row-major) of (2 E E^T - tr(E E^T) I) E, row 9 det E, for
    E = x V[0] + y V[1] + z V[2] + V[3]"""
    e = [np.array([V[0, a], V[1, a], V[2, a], V[3, a]], F) for a in range(9)]      # entry a as a linear form
    G = {}
    for i in range(3):
        for j in range(i, 3):
            G[(i, j)] = _mul11(e[3 * i], e[3 * j], F) + _mul11(e[3 * i + 1], e[3 * j + 1], F) + _mul11(e[3 * i + 2], e[3 * j + 2], F)
            G[(j, i)] = G[(i, j)]
    tr = G[(0, 0)] + G[(1, 1)] + G[(2, 2)]
    L = {(i, j): F(2) * G[(i, j)] - (tr if i == j else F(0)) for i in range(3) for j in range(3)}
    M = np.zeros((10, 20), F)
    for i in range(3):
        for j in range(3):
            c = _mul21(L[(i, 0)], e[j], F) + _mul21(L[(i, 1)], e[3 + j], F) + _mul21(L[(i, 2)], e[6 + j], F)
            M[3 * i + j] = c[_TO_NISTER]
    d = (_mul21(_mul11(e[4], e[8], F) - _mul11(e[5], e[7], F), e[0], F) - _mul21(_mul11(e[3], e[8], F) - _mul11(e[5], e[6], F), e[1], F)
         + _mul21(_mul11(e[3], e[7], F) - _mul11(e[4], e[6], F), e[2], F))
    M[9] = d[_TO_NISTER]
    return M


def eliminate(M, F=np.float64):
    """Gauss-Jordan with partial pivoting (the first largest entry of the column wins) on the first ten columns, in place"""
    for k in range(10):
        p, big = k, F(-1)
        for r in range(k, 10):
            if abs(M[r, k]) > big:
                p, big = r, abs(M[r, k])
        if p != k:
            M[[k, p]] = M[[p, k]]
        M[k, k + 1:] = M[k, k + 1:] / M[k, k]
        M[k, k] = F(1)
        for r in range(10):
            if r != k:
                M[r, k + 1:] = M[r, k + 1:] - M[r, k] * M[k, k + 1:]
                M[r, k] = F(0)
    return M


def _pmul(a, b, F):
    """product of two polynomials, highest power first"""
    out = np.zeros(len(a) + len(b) - 1, F)
    for i in range(len(a)):
        out[i:i + len(b)] = out[i:i + len(b)] + a[i] * b
    return out


def bz_rows(M, F=np.float64):
    """B(z): three rows (k = e - z f, l = g - z h, m = i - z j), each (x: 4 coefficients, y: 4, 1: 5), highest power first"""
    rows = []
    for hi, lo in ((4, 5), (6, 7), (8, 9)):
        a, b = M[hi], M[lo]
        px = np.array([-b[10], a[10] - b[11], a[11] - b[12], a[12]], F)
        py = np.array([-b[13], a[13] - b[14], a[14] - b[15], a[15]], F)
        p1 = np.array([-b[16], a[16] - b[17], a[17] - b[18], a[18] - b[19], a[19]], F)
        rows.append((px, py, p1))
    return rows


def det_poly(B, F=np.float64):
    """det B(z): 11 coefficients, highest power first"""
    (kx, ky, k1), (lx, ly, l1), (mx, my, m1) = B
    return (_pmul(kx, _pmul(ly, m1, F) - _pmul(l1, my, F), F) - _pmul(ky, _pmul(lx, m1, F) - _pmul(l1, mx, F), F)
            + _pmul(k1, _pmul(lx, my, F) - _pmul(ly, mx, F), F))


# ---- step 4: real roots --------------------------------------------------------------------------------------------------------------
def sturm_chain(c, F=np.float64):
    """(11, 11): p_0 = p, p_1 = p', p_{k+1} = -rem(p_{k-1}, p_k), p_k held with the FORMAL degree 10 - k (highest power first, padded
    with zeros behind): a chain whose degrees do not drop one at a time divides by a zero and yields non-finite entries, which
    sign_changes() skips"""
    S = np.zeros((11, 11), F)
    S[0] = c
    for i in range(10):
        S[1, i] = F(10 - i) * c[i]
    for k in range(1, 10):
        a, b = S[k - 1], S[k]
        da, db = 11 - k, 10 - k                                   # coefficient counts minus one = formal degrees + ... (da = deg a)
        q1 = a[0] / b[0]
        t = a[1:da + 1].copy()                                     # a - q1 x b: degree da - 1
        t[:db] = t[:db] - q1 * b[1:db + 1]
        q0 = t[0] / b[0]
        r = t[1:da].copy()                                         # degree da - 2
        r[:db] = r[:db] - q0 * b[1:db + 1]
        S[k + 1, :da - 1] = -r
    return S


def _chain_values(S, x, F):
    v = S[:, 0].copy()
    for i in range(1, 11):
        live = np.arange(11) <= 10 - i                             # p_k has 11 - k coefficients
        v = np.where(live, v * x + S[:, i], v)
    return v


def sign_changes(S, x, F=np.float64):
    """sign changes along the chain at x; zeros and non-finite values are skipped"""
    v = _chain_values(S, x, F)
    n, last = 0, 0
    for k in range(11):
        s = 1 if v[k] > 0 else (-1 if v[k] < 0 else 0)
        if s != 0 and not np.isfinite(v[k]):
            s = 0
        if s != 0:
            if last != 0 and s != last:
                n += 1
            last = s
    return n


def _horner(c, x):
    v, d = c[0], c[0] * 0
    for k in range(1, len(c)):
        d = d * x + v
        v = v * x + c[k]
    return v, d


def real_roots(c, F=np.float64):
    """every real root of the degree-10 polynomial c (highest power first), ascending: Sturm counts inside the Cauchy bound
    (-B, B], B = 1 + max |c_k / c_0|; root j is isolated by bisection on the count (at most ISOLATE_TRIPS halvings, until its
    interval holds one root), refined by REFINE_TRIPS halvings on the sign of p and NEWTON_STEPS Newton steps (a step that is not
    finite or leaves the interval is not taken)"""
    c = np.asarray(c, F)
    if not np.all(np.isfinite(c)) or c[0] == 0:
        return []
    B = F(1) + np.max(np.abs(c[1:] / c[0]))
    if not np.isfinite(B):
        return []
    S = sturm_chain(c, F)
    v_lo = sign_changes(S, -B, F)
    total = v_lo - sign_changes(S, B, F)
    roots = []
    for j in range(min(max(total, 0), 10)):
        lo, hi, n_lo, n_hi = -B, B, 0, total                       # roots in (-B, lo] and in (-B, hi]
        for _ in range(ISOLATE_TRIPS):
            if n_lo == j and n_hi == j + 1:
                break
            mid = (lo + hi) / F(2)
            n_mid = v_lo - sign_changes(S, mid, F)
            if n_mid >= j + 1:
                hi, n_hi = mid, n_mid
            else:
                lo, n_lo = mid, n_mid
        p_lo = _horner(c, lo)[0]
        for _ in range(REFINE_TRIPS):
            mid = (lo + hi) / F(2)
            p_mid = _horner(c, mid)[0]
            if (p_mid > 0) == (p_lo > 0):
                lo = mid
            else:
                hi = mid
        x = (lo + hi) / F(2)
        for _ in range(NEWTON_STEPS):
            v, d = _horner(c, x)
            xn = x - v / d
            if np.isfinite(xn) and lo <= xn <= hi:
                x = xn
        roots.append(x)
    return roots


# ---- steps 5-6: from a root to the candidates -----------------------------------------------------------------------------------------
def _peval(c, z):
    v = c[0]
    for k in range(1, len(c)):
        v = v * z + c[k]
    return v


def essential_of_root(V, B, z, F=np.float64):
    """E (9,) row-major of the root z: x, y from the two rows of B(z) whose 2 x 2 determinant is largest (the first largest of the
    pairs (k, l), (k, m), (l, m))"""
    b = [(_peval(px, z), _peval(py, z), _peval(p1, z)) for px, py, p1 in B]
    best, bd = None, F(-1)
    for r1, r2 in ((0, 1), (0, 2), (1, 2)):
        det = b[r1][0] * b[r2][1] - b[r1][1] * b[r2][0]
        if abs(det) > bd:
            best, bd = (r1, r2, det), abs(det)
    if best is None:
        return np.full(9, np.nan, F)
    r1, r2, det = best
    x = (b[r2][2] * b[r1][1] - b[r1][2] * b[r2][1]) / det
    y = (b[r1][2] * b[r2][0] - b[r2][2] * b[r1][0]) / det
    return x * V[0] + y * V[1] + z * V[2] + V[3]


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], a.dtype)


def horn(E, F=np.float64):
    """the four (R, t) of an essential matrix E (9,), Horn's closed form without an SVD: E scaled to tr(E E^T) = 2, b b^T = I - E E^T
    (b from the row with the largest diagonal entry, the first largest), R = Cof(E) - [b]x E; candidates (b, E), (b, -E), (-b, E),
    (-b, -E) in this order"""
    E = np.asarray(E, F).reshape(3, 3)
    tr = F(0)
    for a in range(3):
        for c in range(3):
            tr = tr + E[a, c] * E[a, c]
    E = E / np.sqrt(tr / F(2))
    G = np.zeros((3, 3), F)
    for a in range(3):
        for c in range(3):
            G[a, c] = (F(1) if a == c else F(0)) - ((E[a, 0] * E[c, 0] + E[a, 1] * E[c, 1]) + E[a, 2] * E[c, 2])
    i = 0
    if G[1, 1] > G[i, i]:
        i = 1
    if G[2, 2] > G[i, i]:
        i = 2
    b = G[i] / np.sqrt(G[i, i])
    cof = np.stack([_cross(E[1], E[2]), _cross(E[2], E[0]), _cross(E[0], E[1])])
    bE = np.stack([_cross(b, E[:, 0]), _cross(b, E[:, 1]), _cross(b, E[:, 2])], axis=1)       # [b]x E, column by column
    Ra, Rb = cof - bE, cof + bE
    return [(Ra, b), (Rb, b), (Rb, -b), (Ra, -b)]


# ---- the distance ----------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def triangulate2(R, t, f1, f2):
    """opengv::triangulation::triangulate2 as csrc/triangulate.hip restates it (tri_triangulate2): the midpoint, in frame 1"""
    f2u = f2 @ R.T
    b0, b1 = _dot(f1, t), _dot(f2u, t)
    a00, a10 = _dot(f1, f1), _dot(f1, f2u)
    a01, a11 = -a10, -_dot(f2u, f2u)
    invdet = 1 / (a00 * a11 - a10 * a01)
    i00, i10, i01, i11 = a11 * invdet, -a10 * invdet, -a01 * invdet, a00 * invdet
    l0, l1 = i00 * b0 + i01 * b1, i10 * b0 + i11 * b1
    return (l0[..., None] * f1 + (t + l1[..., None] * f2u)) / 2


def distances(R, t, f1, f2):
    """d_i = (1 - f1_i . p / |p|) + (1 - f2_i . r / |r|), p = triangulate2, r = R^T (p - t)"""
    with np.errstate(all="ignore"):
        p = triangulate2(R, t, f1, f2)
        r = (p - t) @ R
        return (1 - _dot(f1, p) / np.sqrt(_dot(p, p))) + (1 - _dot(f2, r) / np.sqrt(_dot(r, r)))


# ---- one row -----------------------------------------------------------------------------------------------------------------------------
def solve_five(f1, f2, F=np.float64):
    """every finite essential matrix (9,) of five correspondences, by ascending root; also (V, B, polynomial, roots)"""
    with np.errstate(all="ignore"):
        V = null_space(f1, f2, F)
        M = eliminate(constraints(V, F), F)
        B = bz_rows(M, F)
        c = det_poly(B, F)
        roots = real_roots(c, F)
        Es = [essential_of_root(V, B, z, F) for z in roots]
    return Es, dict(V=V, B=B, poly=c, roots=roots)


def hypothesis(row, bv1, bv2, F=np.float64):
    """(model 3 x 4 [R | t], number of real roots, (root, candidate) chosen) of a sample row; the model is None for an invalid
    row (a repeated or out-of-range index, no real root, no finite candidate)"""
    n = len(bv1)
    row = [int(i) for i in row]
    if min(row) < 0 or max(row) >= n or len(set(row)) != SAMPLE:
        return None, 0, (-1, -1)
    f1, f2 = bv1[row], bv2[row]
    Es, info = solve_five(f1[:5], f2[:5], F)
    best, bests, pick = None, None, (-1, -1)
    with np.errstate(all="ignore"):
        for ri, E in enumerate(Es):
            if not np.all(np.isfinite(E)):
                continue
            for ci, (R, t) in enumerate(horn(E, F)):
                if not (np.all(np.isfinite(R)) and np.all(np.isfinite(t))):
                    continue
                d = distances(R, t, f1, f2)
                s = F(0)
                for j in range(SAMPLE):
                    s = s + d[j]
                if not np.isfinite(s):
                    continue
                if best is None or s < bests:
                    best, bests, pick = np.concatenate([R, t[:, None]], axis=1), s, (ri, ci)
    return best, len(info["roots"]), pick


def prepare(bv1, bv2, samples, F=np.float64):
    """every row's (models, distances over all points, root counts, picks): the part of a search that the loop only reads"""
    bv1, bv2 = np.asarray(bv1, F).reshape(-1, 3), np.asarray(bv2, F).reshape(-1, 3)
    samples = np.asarray(samples, np.int32).reshape(-1, SAMPLE)
    S = len(samples)
    if len(bv1) < SAMPLE:
        return [None] * S, [None] * S, [0] * S, [(-1, -1)] * S
    hyp = [hypothesis(r, bv1, bv2, F) for r in samples]
    models = [h[0] for h in hyp]
    dist = [None if m is None else distances(m[:, :3], m[:, 3], bv1, bv2) for m in models]
    return models, dist, [h[1] for h in hyp], [h[2] for h in hyp]


def search(bv1, bv2, samples, max_iterations, threshold, probability=0.99, F=np.float64, prep=None):
    """The whole call: OpenGV's sac::Ransac loop as p3p_ref.search replays it, with a sample size of 8.  Returns a dict: model
    (12,) (R row-major, t), best_row, score (the inlier count), iterations, rows_consumed, status, n_inliers, outliers (ascending
    int32), trace_valid (S,), trace_score (S,), trace_model (S, 12), consumed_rows (the rows the loop took, in order)."""
    bv1, bv2 = np.asarray(bv1, F).reshape(-1, 3), np.asarray(bv2, F).reshape(-1, 3)
    samples = np.asarray(samples, np.int32).reshape(-1, SAMPLE)
    n, S = len(bv1), len(samples)
    threshold = F(threshold)
    res = dict(model=np.zeros(12, F), best_row=-1, score=F(0), iterations=0, rows_consumed=0, status=0, n_inliers=0,
               outliers=np.zeros(0, np.int32), trace_valid=np.zeros(S, np.uint8), trace_score=np.zeros(S, F),
               trace_model=np.zeros((S, 12), F), consumed_rows=[])
    if n < SAMPLE:
        res["status"] = TOO_FEW_POINTS
        return res
    models, dist = (prep if prep is not None else prepare(bv1, bv2, samples, F))[:2]
    for r in range(S):
        if models[r] is not None:
            res["trace_valid"][r] = 1
            res["trace_score"][r] = F((dist[r] < threshold).sum())
            res["trace_model"][r] = np.concatenate([models[r][:, :3].reshape(9), models[r][:, 3]])
    it, r, best_row, best, k = 0, 0, -1, -1, 1.0
    eps = float(np.finfo(np.float64).eps)
    while it < k and r < S:
        cur = r
        r += 1
        res["consumed_rows"].append(cur)
        if models[cur] is None:
            continue                                               # a skipped row does not count an iteration
        cnt = int(res["trace_score"][cur])
        if cnt > best:                                             # a tie keeps the first
            best, best_row = cnt, cur
            w = cnt / n
            w2 = w * w
            w4 = w2 * w2
            q = min(max(1.0 - w4 * w4, eps), 1.0 - eps)
            k = math.log(1.0 - probability) / math.log(q)
        it += 1
        if it > max_iterations:
            break
    res["iterations"], res["rows_consumed"] = it, r
    if best_row < 0:
        res["status"] = NO_MODEL | FEW_INLIERS
        return res
    d = dist[best_row]
    res["model"] = res["trace_model"][best_row].copy()
    res["best_row"], res["score"] = best_row, res["trace_score"][best_row]
    inl = d < threshold
    res["n_inliers"] = int(inl.sum())
    res["outliers"] = np.nonzero(~inl)[0].astype(np.int32)
    if res["n_inliers"] < MIN_INLIERS:
        res["status"] |= FEW_INLIERS
    return res


def fragile_rows(prep64, prepld, threshold, margin=1e-6):
    """(S,) bool: rows on which float64 and longdouble DECIDE differently (validity, number of real roots, chosen (root,
    candidate), inlier count) or on which a point's d lies within margin * threshold of the threshold"""
    m64, d64, n64, p64 = prep64
    mld, dld, nld, pld = prepld
    out = np.zeros(len(m64), bool)
    for r in range(len(m64)):
        if (m64[r] is None) != (mld[r] is None) or n64[r] != nld[r] or p64[r] != pld[r]:
            out[r] = True
        elif m64[r] is not None:
            a, b = d64[r] < threshold, dld[r] < np.longdouble(threshold)
            near = np.abs(d64[r] - threshold) <= margin * threshold
            out[r] = bool(a.sum() != b.sum() or near.any() or not np.all(np.isfinite(d64[r])))
    return out


def threshold_of(errth, fx, fy):
    """the reference's 2 (1 - cos(atan(errth / focal))), focal the float (fx + fy) / 2, the quotient a float, evaluated in double"""
    focal = np.float32(np.float32(fx) + np.float32(fy))
    focal = np.float32(np.float64(focal) / 2.)
    return 2.0 * (1.0 - math.cos(math.atan(float(np.float32(errth) / focal))))


# ---- scenes --------------------------------------------------------------------------------------------------------------------------
def _rot(rng, ang):
    a = rng.normal(size=3)
    a /= np.sqrt((a * a).sum())
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * K @ K


def make_scene(rng, n, noise_px=0.0, outlier_frac=0.0, focal=460.0, outlier_px=60.0):
    """n points seen by two cameras with a known relative pose x1 = R x2 + t, |t| = 1: (bv1, bv2, R, t, planted outlier mask).
    Noise and outliers displace the normalised image point of camera 2, in pixels of a camera with the given focal length; an
    outlier is displaced ACROSS its epipolar line (along the line it would stay consistent with the essential matrix)."""
    R = _rot(rng, rng.uniform(0.05, 0.4))
    t = rng.normal(size=3)
    t /= np.sqrt((t * t).sum())
    x2 = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(3.0, 8.0, n)], axis=1)
    x1 = x2 @ R.T + t
    bv1 = x1 / np.sqrt((x1 * x1).sum(axis=1))[:, None]
    uv = x2[:, :2] / x2[:, 2:3]
    if noise_px > 0:
        uv = uv + rng.normal(0, noise_px / focal, uv.shape)
    planted = np.zeros(n, bool)
    if outlier_frac > 0:
        k = int(round(outlier_frac * n))
        idx = rng.choice(n, k, replace=False)
        planted[idx] = True
        Em = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R
        line = bv1[idx] @ Em                                       # l . (u, v, 1) = 0: the epipolar line in image 2
        nrm = line[:, :2] / np.sqrt((line[:, :2] ** 2).sum(axis=1))[:, None]
        mag = rng.uniform(20.0, outlier_px, k) / focal * rng.choice([-1.0, 1.0], k)
        uv[idx] += mag[:, None] * nrm
    bv2 = np.concatenate([uv, np.ones((n, 1))], axis=1)
    bv2 /= np.sqrt((bv2 * bv2).sum(axis=1))[:, None]
    return bv1, bv2, R, t, planted
