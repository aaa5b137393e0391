"""The specification of the device P3P pose search (csrc/p3p.hip, ov2_p3p_ransac[_batch]) in numpy: Kneip's P3P on the first three
indices of a sample row, the fourth index picks among its solutions, and OpenGV's LMedS / RANSAC loops are replayed over a sample
table that is an INPUT, so the result is a function of the inputs alone.  OpenGV is not available to this project: the solver and
the two loops are restated from the paper (Kneip, Scaramuzza, Siegwart, CVPR 2011) and from the library's published behaviour, and
nothing here was compared with an OpenGV binary.  The rules at exact equality (strictly smaller penalty, strictly larger count, the
first solution wins a tie on the fourth point) are this project's canonical choice.

Every function takes the float type F (np.float64: the specification; np.longdouble: the same code in extended precision, which
the GPU test uses to measure how far float64 itself is from the exact result)."""
import math

import numpy as np

LMEDS, RANSAC = 0, 1
TOO_FEW_POINTS, NO_MODEL, FEW_INLIERS, NOT_ORTHOGONAL = 1, 2, 4, 8
MAX_POINTS, MAX_ROWS = 2048, 4096
_M64 = (1 << 64) - 1
# A solution must reproduce its own three bearings to this d = 1 - cos.  d is quadratic in the angular error: an accepted root is
# good to ~1e-8 at worst (a near-duplicate, see accept_roots), which is d ~ 1e-15 at ordinary conditioning, next to the few 1e-16
# of the subtraction itself; 1e-12 leaves three digits, and is an angle of 1.4e-6 rad, 1e-3 px at the reference's focal lengths.
BEARING_TOL = 1e-12


# ---- sample table ----------------------------------------------------------------------------------------------------------------
def _splitmix64(seed, j):
    """draw j (0-based) of the counter-based stream of `seed`"""
    z = (seed + (j + 1) * 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def draw_samples(seed, n, rows):
    """rows x 4 int32: every row four distinct indices of [0, n), a slot that repeats an earlier slot of its row is drawn again"""
    if n < 4 or rows < 0:
        raise ValueError("draw_samples: n >= 4 and rows >= 0")
    out = np.zeros((rows, 4), np.int32)
    j = 0
    for r in range(rows):
        k = 0
        while k < 4:
            v = _splitmix64(seed & _M64, j) % n
            j += 1
            if v in out[r, :k]:
                continue
            out[r, k] = v
            k += 1
    return out


# ---- Kneip's P3P -------------------------------------------------------------------------------------------------------------------
def _norm(v):
    return np.sqrt((v * v).sum())


def quartic(f, P, F=np.float64):
    """(coefficients c[0] x^4 + ... + c[4], the intermediate frame) of the three correspondences f (3x3 bearings), P (3x3 points)"""
    f1, f2, f3 = f[0], f[1], f[2]
    P1, P2, P3 = P[0], P[1], P[2]

    def frame(a, b):
        e3 = np.cross(a, b)
        e3 = e3 / _norm(e3)
        return np.stack([a, np.cross(e3, a), e3])
    T = frame(f1, f2)
    g3 = T @ f3
    if g3[2] > 0:
        f1, f2 = f2, f1
        P1, P2 = P2, P1
        T = frame(f1, f2)
        g3 = T @ f3
    d12 = _norm(P2 - P1)
    n1 = (P2 - P1) / d12
    n3 = np.cross(n1, P3 - P1)
    n3 = n3 / _norm(n3)
    N = np.stack([n1, np.cross(n3, n1), n3])
    p = N @ (P3 - P1)
    p1, p2 = p[0], p[1]
    phi1, phi2 = g3[0] / g3[2], g3[1] / g3[2]
    cb = (f1 * f2).sum()
    b = np.sqrt(F(1) / (F(1) - cb * cb) - F(1))
    if cb < 0:
        b = -b
    f1_2, f2_2 = phi1 * phi1, phi2 * phi2
    p1_2 = p1 * p1; p1_3 = p1_2 * p1; p1_4 = p1_3 * p1
    p2_2 = p2 * p2; p2_3 = p2_2 * p2; p2_4 = p2_3 * p2
    d_2, b_2 = d12 * d12, b * b
    c = np.zeros(5, F)
    c[0] = -f2_2 * p2_4 - p2_4 * f1_2 - p2_4
    c[1] = F(2) * p2_3 * d12 * b + F(2) * f2_2 * p2_3 * d12 * b - F(2) * phi2 * p2_3 * phi1 * d12
    c[2] = (-f2_2 * p2_2 * p1_2 - f2_2 * p2_2 * d_2 * b_2 - f2_2 * p2_2 * d_2 + f2_2 * p2_4 + p2_4 * f1_2 + F(2) * p1 * p2_2 * d12
            + F(2) * phi1 * phi2 * p1 * p2_2 * d12 * b - p2_2 * p1_2 * f1_2 + F(2) * p1 * p2_2 * f2_2 * d12 - p2_2 * d_2 * b_2
            - F(2) * p1_2 * p2_2)
    c[3] = (F(2) * p1_2 * p2 * d12 * b + F(2) * phi2 * p2_3 * phi1 * d12 - F(2) * f2_2 * p2_3 * d12 * b
            - F(2) * p1 * p2 * d_2 * b)
    c[4] = (-F(2) * phi2 * p2_2 * phi1 * p1 * d12 * b + f2_2 * p2_2 * d_2 + F(2) * p1_3 * d12 - p1_2 * d_2 + f2_2 * p2_2 * p1_2
            - p1_4 - F(2) * f2_2 * p2_2 * p1 * d12 + p2_2 * f1_2 * p1_2 + f2_2 * p2_2 * d_2 * b_2)
    return c, dict(T=T, N=N, P1=P1, p1=p1, p2=p2, phi1=phi1, phi2=phi2, d12=d12, b=b)


def _poly(c, x):
    """(p(x), p'(x), sum |c_k| |x|^k) by Horner"""
    ax = abs(x)
    v, d, m = c[0], c[0] * 0, abs(c[0])
    for k in range(1, 5):
        d = d * x + v
        v = v * x + c[k]
        m = m * ax + abs(c[k])
    return v, d, m


def accept_roots(c, F=np.float64):
    """the acceptance rule: each candidate's real part, two Newton steps, |x| <= 1 and |p(x)| <= 1e-9 sum |c_k||x|^k.  The
    candidates are the four ROOTS of the quartic, complex ones included (here: the companion matrix's eigenvalues; on the device:
    Ferrari's closed form polished by complex Newton steps).  Where they start matters: the real part of a complex pair that lies
    next to a real root is carried by the two steps to within ~1e-8 of that root, passes the residual test and stays in the set as
    a near-duplicate, so an implementation that polished real parts any further would return other numbers."""
    if not np.all(np.isfinite(c)) or c[0] == 0:
        return []
    try:
        cand = np.roots(np.asarray(c, np.float64))
    except np.linalg.LinAlgError:
        return []
    out = []
    for z in cand:
        x = F(z.real)
        for _ in range(2):
            v, d, _m = _poly(c, x)
            x = x - v / d
        v, d, m = _poly(c, x)
        if abs(x) <= 1 and abs(v) <= F(1e-9) * m:
            out.append(x)
    return out


def pose_of_root(x, g, F=np.float64):
    """(Rwc, C) of one accepted root cos(theta) = x"""
    p1, p2, phi1, phi2, d12, b = g["p1"], g["p2"], g["phi1"], g["phi2"], g["d12"], g["b"]
    cot = (-phi1 * p1 / phi2 - x * p2 + d12 * b) / (-phi1 * x * p2 / phi2 + p1 - d12)
    ct = x
    st = np.sqrt(F(1) - x * x)
    sa = np.sqrt(F(1) / (cot * cot + F(1)))
    ca = np.sqrt(F(1) - sa * sa)
    if cot < 0:
        ca = -ca
    k = d12 * (sa * b + ca)
    C = np.array([ca * k, ct * sa * k, st * sa * k], F)
    C = g["P1"] + g["N"].T @ C
    Q = np.array([[-ca, -sa * ct, -sa * st], [sa, -ca * ct, -ca * st], [F(0), -st, ct]], F)
    R = g["N"].T @ Q.T @ g["T"]
    return R, C


def kneip(f, P, F=np.float64):
    """every accepted solution (Rwc, C) of three correspondences: the pose of an accepted root that also reproduces its three
    bearings, d <= BEARING_TOL for each.  The quartic alone does not guarantee that: the elimination squares sin(theta) away, so
    some roots belong to the mirrored configuration (point 3 off its bearing), and alpha + beta > pi puts the centre beyond
    point 1 or 2 (d = 2 there); 53 of 606 accepted roots of random scenes are of these kinds.  Kneip's solver as published
    returns them and leaves them to the disambiguation; here they are not solutions."""
    f, P = np.asarray(f, F), np.asarray(P, F)
    out = []
    with np.errstate(all="ignore"):
        c, g = quartic(f, P, F)
        for x in accept_roots(c, F):
            R, C = pose_of_root(x, g, F)
            if np.all(distances(R, C, f, P) <= BEARING_TOL):         # a NaN fails
                out.append((R, C))
    return out


def distances(R, C, bv, X):
    """d_i = max(0, 1 - bv_i . v / |v|), v = R^T (X_i - C); a NaN (X_i == C) counts as 0"""
    with np.errstate(all="ignore"):
        v = (X - C) @ R
        v = v / np.sqrt((v * v).sum(axis=1))[:, None]
        d = 1 - (bv * v).sum(axis=1)
    return np.where(d > 0, d, d.dtype.type(0))


def hypothesis(row, bv, X, F=np.float64):
    """the model (3x4: Rwc | C) of a sample row, or None when the row is invalid"""
    n = len(bv)
    row = [int(i) for i in row]
    if min(row) < 0 or max(row) >= n or len(set(row)) != 4:
        return None
    best, bestd = None, None
    for R, C in kneip(bv[row[:3]], X[row[:3]], F):
        d = distances(R, C, bv[row[3]:row[3] + 1], X[row[3]:row[3] + 1])[0]
        if best is None or d < bestd:
            best, bestd = np.concatenate([R, C[:, None]], axis=1), d
    if best is None or not np.all(np.isfinite(best)):
        return None
    return best


def penalty(d):
    """LMedS: the median of sqrt(d)"""
    s = np.sort(d)
    mid = len(s) // 2
    if len(s) % 2:
        return np.sqrt(s[mid])
    return (np.sqrt(s[mid - 1]) + np.sqrt(s[mid])) / 2


def is_orthogonal(R):
    """Sophus::isOrthogonal (rotation_matrix.hpp): Frobenius norm of R R^T - I below Constants<double>::epsilon() = 1e-10"""
    E = R @ R.T - np.eye(3, dtype=R.dtype)
    return bool(np.sqrt((E * E).sum()) < 1e-10)


def prepare(bv, X, samples, F=np.float64):
    """(models, distances) of every row of the table (None for an invalid row): the part of a search that does not depend on
    the mode, so that tests run both loops on one evaluation"""
    bv, X = np.asarray(bv, F).reshape(-1, 3), np.asarray(X, F).reshape(-1, 3)
    samples = np.asarray(samples, np.int32).reshape(-1, 4)
    if len(bv) < 4:
        return [None] * len(samples), [None] * len(samples)
    models = [hypothesis(r, bv, X, F) for r in samples]
    return models, [None if m is None else distances(m[:, :3], m[:, 3], bv, X) for m in models]


def search(bv, X, samples, mode, max_iterations, threshold, probability=0.99, F=np.float64, prep=None):
    """The whole call.  Returns a dict: model (12,), best_row, score (penalty or count), iterations, rows_consumed, status,
    n_inliers, outliers (ascending int32), trace_valid (S,), trace_score (S,) (every row, whether the loop reached it or not),
    and the two margins the GPU test reads: gap (relative distance between the best and the second-best score among the rows
    the loop counted; equal inlier counts are left out) and th_margin (the smallest |d_i - threshold| / threshold over the winning model's points).  prep: the
    result of prepare() for the same bv, X, samples and F."""
    bv, X = np.asarray(bv, F).reshape(-1, 3), np.asarray(X, F).reshape(-1, 3)
    samples = np.asarray(samples, np.int32).reshape(-1, 4)
    n, S = len(bv), len(samples)
    threshold = F(threshold)
    res = dict(model=np.zeros(12, F), best_row=-1, score=F(0), iterations=0, rows_consumed=0, status=0, n_inliers=0,
               outliers=np.zeros(0, np.int32), trace_valid=np.zeros(S, np.uint8), trace_score=np.zeros(S, F), gap=np.inf,
               th_margin=np.inf)
    if n < 4:
        res["status"] = TOO_FEW_POINTS
        return res
    models, dist = prep if prep is not None else prepare(bv, X, samples, F)
    for r in range(S):
        if models[r] is not None:
            res["trace_valid"][r] = 1
            res["trace_score"][r] = penalty(dist[r]) if mode == LMEDS else F((dist[r] < threshold).sum())
    it, r, best_row, counted = 0, 0, -1, []
    if mode == LMEDS:
        best = np.inf
        while it < max_iterations and r < S:
            cur = r
            r += 1
            if models[cur] is None:
                continue
            counted.append(cur)
            if res["trace_score"][cur] < best:
                best, best_row = res["trace_score"][cur], cur
            it += 1
    else:
        best, k = -1, 1.0
        eps = float(np.finfo(np.float64).eps)
        while it < k and r < S:
            cur = r
            r += 1
            if models[cur] is None:
                continue
            counted.append(cur)
            cnt = int(res["trace_score"][cur])
            if cnt > best:
                best, best_row = cnt, cur
                w = cnt / n
                q = min(max(1.0 - w * w * w * w, eps), 1.0 - eps)
                k = math.log(1.0 - probability) / math.log(q)
            it += 1
            if it > max_iterations:
                break
    res["iterations"], res["rows_consumed"] = it, r
    if best_row < 0:
        res["status"] = NO_MODEL | FEW_INLIERS
        return res
    m, d = models[best_row], dist[best_row]
    res["model"] = np.concatenate([m[:, :3].reshape(9), m[:, 3]])
    res["best_row"], res["score"] = best_row, res["trace_score"][best_row]
    inl = d < threshold
    res["n_inliers"] = int(inl.sum())
    res["outliers"] = np.nonzero(~inl)[0].astype(np.int32)
    if res["n_inliers"] < 5:
        res["status"] |= FEW_INLIERS
    if not is_orthogonal(m[:, :3]):
        res["status"] |= NOT_ORTHOGONAL
    sc = np.array([float(res["trace_score"][c]) for c in counted if c != best_row])
    b = float(res["score"])
    if mode == RANSAC:                 # counts are integers: an exact tie is a tie for every implementation, the first row keeps it
        sc = sc[sc != b]
    if len(sc):
        res["gap"] = float(np.min(np.abs(sc - b)) / max(abs(b), 1e-300))
    res["th_margin"] = float(np.min(np.abs(d - threshold)) / threshold)
    return res


def threshold_of(errth, fx, fy):
    """the reference's 1 - cos(atan(errth / focal)), focal the float (fx + fy) / 2, evaluated in double"""
    focal = np.float32(np.float32(fx) + np.float32(fy))
    focal = np.float32(np.float64(focal) / 2.)
    return 1.0 - math.cos(math.atan(float(np.float32(errth) / focal)))


# ---- scenes --------------------------------------------------------------------------------------------------------------------------
def _rot(rng, ang):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * K @ K


def make_scene(rng, n, noise_px=0.0, outlier_frac=0.0, focal=460.0, outlier_px=60.0):
    """n points in front of a camera with a known pose: (bv, X, Rwc, C, planted outlier mask).  Noise and outliers are
    displacements of the normalised image point, in pixels of a camera with the given focal length."""
    R = _rot(rng, rng.uniform(0.1, 1.0))
    C = rng.uniform(-2, 2, 3)
    pc = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(2.0, 8.0, n)], axis=1)
    X = pc @ R.T + C
    uv = pc[:, :2] / pc[:, 2:3]
    if noise_px > 0:
        uv = uv + rng.normal(0, noise_px / focal, uv.shape)
    planted = np.zeros(n, bool)
    if outlier_frac > 0:
        k = int(round(outlier_frac * n))
        idx = rng.choice(n, k, replace=False)
        planted[idx] = True
        ang = rng.uniform(0, 2 * math.pi, k)
        mag = rng.uniform(20.0, outlier_px, k) / focal
        uv[idx] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], axis=1)
    bv = np.concatenate([uv, np.ones((n, 1))], axis=1)
    bv /= np.linalg.norm(bv, axis=1)[:, None]
    return bv, X, R, C, planted


def dedup_rows(samples):
    """the table without the rows whose first three indices (as a set) and fourth index repeat an earlier row: the same triple
    twice gives exactly equal scores"""
    seen, keep = set(), []
    for r in samples:
        key = tuple(sorted(int(i) for i in r[:3]))
        if key in seen:
            continue
        seen.add(key)
        keep.append(r)
    return np.asarray(keep, np.int32).reshape(-1, 4)
