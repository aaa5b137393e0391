"""The specification of the device pose-graph solver (ov2_pose_graph_solve, ov2slam_amd/csrc/posegraph.hip) in numpy, generic over the
dtype (float64, numpy.longdouble): LeftSE3RelativePoseError as the reference's src/ceres_parametrization.cpp:30-102 writes it (Sophus
SE(3) log, the approximate Jacobians "adapted from Strasdat" restated, not derived), SE3LeftParameterization::Plus, the block-
tridiagonal normal equations, an exact block Cholesky solve of (J^T J + D^2) y = J^T r, Ceres' trust-region loop in the order of
SURVEY.md A9 / Appendix D with the options of Optimizer::localPoseGraph / fullPoseGraph, the two problem builders
(src/optimizer.cpp:2373-2424, :2794-2814), the rigid moves after the solve (:2476-2585) and a scene generator.

Everything per edge is vectorised over the edges; only the block recurrence of the linear solve is a Python loop over the poses.
tests/test_posegraph_reference.py pins the factor and Plus to the reference's compiled code."""
import numpy as np

MAX_POSES, MAX_EDGES = 16384, 32768
TERM_NO_CONVERGENCE, TERM_FUNCTION_TOL, TERM_PARAMETER_TOL, TERM_GRADIENT_TOL, TERM_MIN_RADIUS, TERM_INVALID_STEPS, TERM_FAILURE = range(7)
EPS = 1e-10                        # Sophus::Constants<double>::epsilon()

LOCAL_OPTIONS = dict(max_iter=10, function_tolerance=1e-4)         # src/optimizer.cpp:2441-2446
FULL_OPTIONS = dict(max_iter=100, function_tolerance=1e-6)         # :2820-2825
CERES_DEFAULTS = dict(gradient_tolerance=1e-10, parameter_tolerance=1e-8, initial_radius=1e4, max_radius=1e16, min_radius=1e-32,
                      min_lm_diagonal=1e-6, max_lm_diagonal=1e32, min_relative_decrease=1e-3, jacobi_scaling=True,
                      max_consecutive_invalid_steps=5)


# A finite, accepted initial_radius under which every linear solve fails: diag / radius overflows in float64 (diag >= min_lm_diagonal
# = 1e-6 against a radius of 1e-310 and below), the first pivot is inf, the step is invalid; the radius goes 1e-310, 5e-311, 1.25e-311,
# 1.5625e-312, 9.765625e-314 and the fifth invalid step in a row ends the solve.  A FAILED solve (not a step without descent) is
# Ceres' FAILURE: the input poses come back.  In longdouble the quotient (1e304) is representable and the solve succeeds, so the two
# precisions do NOT decide alike here: only decisions and copied values are compared on this case.
DENORMAL_RADIUS = dict(initial_radius=1e-310, min_radius=0.0, function_tolerance=0.0, parameter_tolerance=0.0, gradient_tolerance=0.0)
DENORMAL_RADIUS_SEED, DENORMAL_RADIUS_N = 105, 5


def denormal_radius_scene():
    return make_local_scene(np.random.default_rng(DENORMAL_RADIUS_SEED), DENORMAL_RADIUS_N)


def options(full=False, **kw):
    o = dict(CERES_DEFAULTS)
    o.update(FULL_OPTIONS if full else LOCAL_OPTIONS)
    o.update(kw)
    return o


# ----------------------------------------------------------------------------------------------------------- SE(3), batched: (q (n, 4), t (n, 3))
def _norm_q(q):
    return q / np.sqrt((q * q).sum(-1, keepdims=True))


def load(P, dt=np.float64):
    """(n, 7) [t q] -> (q, t) with q normalised (Sophus::SE3d(q, t))"""
    P = np.asarray(P, dt).reshape(-1, 7)
    return _norm_q(P[:, 3:]), P[:, :3].copy()


def store(T):
    return np.concatenate([T[1], T[0]], axis=1)


def quat_to_R(q):
    q = _norm_q(q)
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    R = np.empty((len(q), 3, 3), q.dtype)
    R[:, 0, 0] = 1 - (tyy + tzz); R[:, 0, 1] = txy - twz; R[:, 0, 2] = txz + twy
    R[:, 1, 0] = txy + twz; R[:, 1, 1] = 1 - (txx + tzz); R[:, 1, 2] = tyz - twx
    R[:, 2, 0] = txz - twy; R[:, 2, 1] = tyz + twx; R[:, 2, 2] = 1 - (txx + tyy)
    return R


def rot(q, v):
    return np.einsum("nij,nj->ni", quat_to_R(q), v)


def mul(A, B):
    """Sophus SE3 product: the quaternion product of so3.hpp:329-343 renormalised, t = ta + Ra tb"""
    (a, ta), (b, tb) = A, B
    ax, ay, az, aw = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    bx, by, bz, bw = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    q = np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                  aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], axis=1)
    return _norm_q(q), ta + rot(a, tb)


def inv(A):
    q, t = A
    qc = q * np.array([-1, -1, -1, 1], q.dtype)
    return qc, rot(qc, -t)


def hat(v):
    H = np.zeros((len(v), 3, 3), v.dtype)
    H[:, 0, 1] = -v[:, 2]; H[:, 0, 2] = v[:, 1]; H[:, 1, 0] = v[:, 2]; H[:, 1, 2] = -v[:, 0]; H[:, 2, 0] = -v[:, 1]; H[:, 2, 1] = v[:, 0]
    return H


def log(T):
    """Sophus SE3::log (se3.hpp:223-256, so3.hpp:247-290): (n, 6) [rho; omega]"""
    q, t = T
    dt = q.dtype.type
    sn = (q[:, :3] * q[:, :3]).sum(1); w = q[:, 3]
    small = sn < dt(EPS) * dt(EPS)
    with np.errstate(all="ignore"):
        n = np.sqrt(np.where(small, dt(1), sn))
        pi = dt(4) * np.arctan(dt(1))
        k_big = np.where(np.abs(w) < dt(EPS), np.where(w > 0, pi, -pi) / n, dt(2) * np.arctan(n / np.where(w == 0, dt(1), w)) / n)
        k_small = dt(2) / w - (dt(2) / dt(3)) * sn / (w * (w * w))
    k = np.where(small, k_small, k_big)
    theta = np.where(small, dt(2) * sn / w, k * n)
    om = k[:, None] * q[:, :3]
    Om = hat(om)
    tiny = np.abs(theta) < dt(EPS)
    th = np.where(tiny, dt(1), theta)
    h = dt(0.5) * th
    c = np.where(tiny, dt(1) / dt(12), (dt(1) - th * np.cos(h) / (dt(2) * np.sin(h))) / (th * th))
    Vinv = np.eye(3, dtype=q.dtype)[None] - dt(0.5) * Om + c[:, None, None] * (Om @ Om)
    return np.concatenate([np.einsum("nij,nj->ni", Vinv, t), om], axis=1)


def adj(T):
    """SE3::Adj (se3.hpp:103-111): [[R, hat(t) R], [0, R]]"""
    q, t = T
    R = quat_to_R(q)
    A = np.zeros((len(q), 6, 6), q.dtype)
    A[:, :3, :3] = R; A[:, 3:, 3:] = R; A[:, :3, 3:] = hat(t) @ R
    return A


def plus(P, delta):
    """SE3LeftParameterization::Plus: Exp(delta) T (se3left_parametrization.hpp:41-60, se3.hpp:763-784, so3.hpp:585-621)"""
    dt = P.dtype.type
    a = np.asarray(delta, P.dtype).reshape(-1, 6)
    om = a[:, 3:]
    tsq = (om * om).sum(1)
    small = tsq < dt(EPS) * dt(EPS)
    theta = np.where(small, dt(0), np.sqrt(tsq))
    th = np.where(small, dt(1), theta)
    t4 = tsq * tsq
    imag = np.where(small, dt(0.5) - tsq / dt(48) + t4 / dt(3840), np.sin(dt(0.5) * th) / th)
    real = np.where(small, dt(1) - tsq / dt(8) + t4 / dt(384), np.cos(dt(0.5) * th))
    qe = np.concatenate([imag[:, None] * om, real[:, None]], axis=1)
    O = hat(om)
    tq = np.where(small, dt(1), tsq)
    V = np.eye(3, dtype=P.dtype)[None] + ((dt(1) - np.cos(th)) / tq)[:, None, None] * O + ((th - np.sin(th)) / (tq * th))[:, None, None] * (O @ O)
    V = np.where((theta < dt(EPS))[:, None, None], quat_to_R(qe), V)
    E = (qe, np.einsum("nij,nj->ni", V, a[:, :3]))
    return store(mul(E, load(P, P.dtype)))


def edge_eval(Pi, Pj, Tm, si, jac=True):
    """LeftSE3RelativePoseError::Evaluate on m edges: r (m, 6), and the local Jacobians J0, J1 (m, 6, 6) (the first six columns of
    the reference's 6x7 blocks; SE3LeftParameterization::ComputeJacobian = [I6; 0]).  si = 1 / sigma (sqrt_info = si I)."""
    dtp = np.asarray(Pi).dtype
    dt = dtp.type
    T0, T1, M = load(Pi, dtp), load(Pj, dtp), load(Tm, dtp)
    Tc1w = inv(T1)
    err = mul(mul(Tc1w, T0), M)
    v = log(err)
    si = np.asarray(si, dtp).reshape(-1, 1)
    r = si * v
    if not jac:
        return r, None, None
    W, P = hat(v[:, 3:]), hat(v[:, :3])
    Jc = np.zeros((len(v), 6, 6), dtp)
    Jc[:, :3, :3] = W; Jc[:, :3, 3:] = P; Jc[:, 3:, 3:] = W
    I6 = np.eye(6, dtype=dtp)[None]
    J0 = si[:, :, None] * ((I6 - dt(0.5) * Jc) @ adj(Tc1w))
    J1 = -si[:, :, None] * ((I6 + dt(0.5) * Jc) @ adj(inv(mul(T0, M))))
    return r, J0, J1


# ----------------------------------------------------------------------------------------------------------- problems
def inv_pose(T, dt=np.float64):
    return store(inv(load(T, dt)))[0]


def mul_pose(A, B, dt=np.float64):
    return store(mul(load(A, dt), load(B, dt)))[0]


def local_pose_graph(kf_poses, loop_edge_T):
    """src/optimizer.cpp:2373-2424.  kf_poses: Twc per keyframe id from the loop keyframe to the new keyframe, None where the map
    has no keyframe of that id (:2391-2396: skipped; a missing NEW keyframe makes the reference return false -> None here).
    Returns dict(poses, pose_const, edge_i, edge_j, edge_T, ids) with indices into the compacted pose array."""
    if kf_poses[-1] is None:
        return None
    ids = [k for k, p in enumerate(kf_poses) if p is not None]
    assert ids and ids[0] == 0, "the loop keyframe itself exists (:2366-2371 moves on to the first id that does)"
    poses = np.array([kf_poses[k] for k in ids], np.float64).reshape(-1, 7)
    n = len(poses)
    ei, ej, eT = [], [], []
    for k in range(1, n):
        ei.append(k - 1); ej.append(k); eT.append(mul_pose(inv_pose(poses[k - 1]), poses[k]))        # Tcicj = Tciw * Twcj
    ei.append(0); ej.append(n - 1); eT.append(np.asarray(loop_edge_T, np.float64))                     # Tloop_new (:2421-2424)
    const = np.zeros(n, np.uint8); const[0] = 1
    return dict(poses=poses, pose_const=const, edge_i=np.array(ei, np.int32), edge_j=np.array(ej, np.int32),
                edge_T=np.array(eT).reshape(-1, 7), ids=ids)


def full_pose_graph(vTwc, vTpc, viskf):
    """src/optimizer.cpp:2794-2814"""
    vTwc = np.asarray(vTwc, np.float64).reshape(-1, 7); vTpc = np.asarray(vTpc, np.float64).reshape(-1, 7)
    n = len(vTwc)
    return dict(poses=vTwc, pose_const=np.asarray(viskf, bool).astype(np.uint8), edge_i=np.arange(0, n - 1, dtype=np.int32),
                edge_j=np.arange(1, n, dtype=np.int32), edge_T=vTpc[1:].copy())


class Structure:
    """What the solver derives from a problem: the variable poses in index order, the edges that touch one (an edge between two
    constant poses takes no part), the segments of the block-tridiagonal normal matrix."""

    def __init__(self, prob):
        const = np.asarray(prob["pose_const"]).astype(bool)
        n = len(const)
        self.vidx = np.full(n, -1, np.int64)
        self.vpose = np.nonzero(~const)[0]
        self.vidx[self.vpose] = np.arange(len(self.vpose))
        ei, ej = np.asarray(prob["edge_i"], np.int64), np.asarray(prob["edge_j"], np.int64)
        assert ((ei >= 0) & (ei < n) & (ej >= 0) & (ej < n) & (ei != ej)).all()
        ki, kj = self.vidx[ei], self.vidx[ej]
        self.act = np.nonzero((ki >= 0) | (kj >= 0))[0]
        self.ei, self.ej, self.ki, self.kj = ei[self.act], ej[self.act], ki[self.act], kj[self.act]
        both = (self.ki >= 0) & (self.kj >= 0)
        if (np.abs(self.ki - self.kj)[both] != 1).any():
            raise ValueError("an edge joins two variable poses that are not neighbours")
        self.n_var = len(self.vpose)
        self.in_prog = np.zeros(self.n_var, bool)
        self.in_prog[self.ki[self.ki >= 0]] = True; self.in_prog[self.kj[self.kj >= 0]] = True
        coupled = np.zeros(self.n_var + 1, bool)
        coupled[np.minimum(self.ki, self.kj)[both]] = True
        self.segments = []
        k = 0
        while k < self.n_var:
            if not self.in_prog[k]:
                k += 1; continue
            e = k
            while coupled[e]:
                e += 1
            self.segments.append((k, e + 1)); k = e + 1
        sig = prob.get("edge_sigma")
        self.si = np.ones(len(self.act)) if sig is None else 1.0 / np.asarray(sig, np.float64)[self.act]
        self.eT = np.asarray(prob["edge_T"], np.float64).reshape(-1, 7)[self.act]


def residuals(S, x, jac=True):
    dt = x.dtype
    return edge_eval(x[S.ei], x[S.ej], S.eT.astype(dt), S.si.astype(dt), jac)


def cost(prob, poses, dt=np.float64):
    """0.5 sum r^2 over the edges of the program at `poses`"""
    S = Structure(prob)
    r, _, _ = residuals(S, np.asarray(poses, dt).reshape(-1, 7), False)
    return dt(0.5) * (r * r).sum()


def gradient(prob, poses, dt=np.float64):
    """J^T r (un-scaled, tangent space) over the variable poses of the program at `poses`, flattened"""
    S = Structure(prob)
    r, J0, J1 = residuals(S, np.asarray(poses, dt).reshape(-1, 7))
    return assemble(S, J0, J1, r, np.ones((S.n_var, 6), dt))[3][S.in_prog].ravel()


def assemble(S, J0, J1, r, scale):
    """Blocks of Js^T Js (Js = J scale): diagonal H (n_var, 6, 6), coupling C[k] of variable k to k + 1, b = Js^T r, and g = J^T r"""
    dt = r.dtype
    H = np.zeros((S.n_var, 6, 6), dt); Cc = np.zeros((S.n_var, 6, 6), dt); b = np.zeros((S.n_var, 6), dt); g = np.zeros((S.n_var, 6), dt)
    mi, mj = S.ki >= 0, S.kj >= 0
    Js0 = J0 * scale[np.maximum(S.ki, 0)][:, None, :]; Js1 = J1 * scale[np.maximum(S.kj, 0)][:, None, :]
    for J, Js, m, k in ((J0, Js0, mi, S.ki), (J1, Js1, mj, S.kj)):
        np.add.at(H, k[m], np.einsum("nqa,nqc->nac", Js[m], Js[m]))
        np.add.at(b, k[m], np.einsum("nqa,nq->na", Js[m], r[m]))
        np.add.at(g, k[m], np.einsum("nqa,nq->na", J[m], r[m]))
    both = mi & mj
    fwd = both & (S.ki < S.kj); bwd = both & (S.kj < S.ki)
    np.add.at(Cc, S.ki[fwd], np.einsum("nqa,nqc->nac", Js0[fwd], Js1[fwd]))
    np.add.at(Cc, S.kj[bwd], np.einsum("nqa,nqc->nac", Js1[bwd], Js0[bwd]))
    return H, Cc, b, g


def _chol(A):
    n = len(A)
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not (d > 0 and np.isfinite(d)):
            return None
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _fwd(L, B):
    X = np.array(B, copy=True)
    for i in range(len(L)):
        X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def _bwd(L, B):
    X = np.array(B, copy=True)
    for i in range(len(L) - 1, -1, -1):
        X[i] = (X[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


def block_tridiagonal_solve(A, Cc, b, segments):
    """Exact solve of the symmetric block-tridiagonal system with diagonal blocks A[k] and coupling blocks Cc[k] (rows k, columns
    k + 1) over each segment [k0, k1): block Cholesky L_k L_k^T = A_k - W_{k-1}^T W_{k-1}, W_k = L_k^-1 C_k.  None if a pivot fails."""
    y = np.zeros_like(b)
    for k0, k1 in segments:
        Ls, Ws = [], []
        W = z = None
        for k in range(k0, k1):
            Ak, v = A[k], b[k]
            if k > k0:
                Ak = Ak - W.T @ W; v = v - W.T @ z
            L = _chol(Ak)
            if L is None:
                return None
            last = k + 1 == k1
            X = _fwd(L, v[:, None] if last else np.concatenate([v[:, None], Cc[k]], axis=1))
            z = X[:, 0]; W = None if last else X[:, 1:]
            y[k] = z; Ls.append(L); Ws.append(W)
        for k in range(k1 - 1, k0 - 1, -1):
            v = y[k]
            if k + 1 < k1:
                v = v - Ws[k - k0] @ y[k + 1]
            y[k] = _bwd(Ls[k - k0], v)
    return y


def lm_step_accepted(radius, rel, max_radius):
    """LevenbergMarquardtStrategy::StepAccepted -> (radius, decrease_factor)"""
    t = 2.0 * rel - 1.0
    return min(max_radius, radius / max(1.0 / 3.0, 1.0 - t * t * t)), 2.0


def lm_step_rejected(radius, decrease_factor):
    return radius / decrease_factor, decrease_factor * 2.0


def lm_radius_sequence(radius, max_radius, events):
    """the radii after each ("accept", step quality) / ("reject", _) event, through the two functions the loop uses"""
    df, out = 2.0, []
    for what, q in events:
        radius, df = lm_step_accepted(radius, q, max_radius) if what == "accept" else lm_step_rejected(radius, df)
        out.append(radius)
    return out


def solve(prob, opts=None, dt=np.float64):
    """Ceres' TrustRegionMinimizer with LM / an exact normal-equation solve, order of SURVEY.md A9 / Appendix D.  Returns a dict:
    poses, iterations, num_successful_steps, initial_cost, final_cost, termination, trace (the iteration summaries Ceres pushes:
    entry 0 the start; an iteration that ends the solve inside the loop is not recorded), decisions (a string: o accepted,
    r rejected, i invalid, then the exit: f function / p parameter / g gradient / m max iterations / s min radius / x invalid steps)."""
    o = opts or options()
    S = Structure(prob)
    x = np.asarray(prob["poses"], np.float64).reshape(-1, 7).astype(dt)
    if not S.in_prog.any():
        return dict(poses=x.copy(), iterations=0, num_successful_steps=0, initial_cost=dt(0), final_cost=dt(0),
                    termination=TERM_FUNCTION_TOL, trace=[], decisions="")
    T = dt
    f = lambda v: float(v)
    prog = S.in_prog
    pp = S.vpose[prog]                                             # poses in the program
    scale = np.ones((S.n_var, 6), dt)
    r, J0, J1 = residuals(S, x)
    x_cost = T(0.5) * (r * r).sum()
    H, Cc, b, g = assemble(S, J0, J1, r, scale)
    if o["jacobi_scaling"]:
        scale = T(1) / (T(1) + np.sqrt(H[:, np.arange(6), np.arange(6)]))
        H, Cc, b, g = assemble(S, J0, J1, r, scale)
    gmax = np.abs(g[prog]).max()
    initial_cost = minimum_cost = x_cost
    x_norm, radius, df = T(-1), T(o["initial_radius"]), T(2)
    num_invalid = iteration = n_success = n_steps = 0
    ev_min = ev_cur = ev_ref = ev_cand = x_cost
    ev_acc_ref = ev_acc_cand = T(0)
    ev_nonmono = 0
    step_successful = True
    cur = dict(iteration=0, step_is_valid=1, step_is_successful=1, cost=f(x_cost), cost_change=0.0, gradient_max_norm=f(gmax), step_norm=0.0,
               relative_decrease=0.0)
    trace, dec = [], ""
    while True:
        if step_successful:
            n_success += 1
            minimum_cost = min(minimum_cost, x_cost)
        cur["trust_region_radius"] = f(radius)
        trace.append(dict(cur))
        if iteration >= o["max_iter"]:
            term = TERM_NO_CONVERGENCE; dec += "m"; break
        if step_successful and gmax <= o["gradient_tolerance"]:
            term = TERM_GRADIENT_TOL; dec += "g"; break
        if radius <= o["min_radius"]:
            term = TERM_MIN_RADIUS; dec += "s"; break
        iteration += 1
        step_successful = False
        n_steps += 1
        cur = dict(iteration=iteration, step_is_valid=0, step_is_successful=0, cost=0.0, cost_change=0.0, gradient_max_norm=f(gmax),
                   step_norm=0.0, relative_decrease=0.0)
        diag = np.clip(H[:, np.arange(6), np.arange(6)], T(o["min_lm_diagonal"]), T(o["max_lm_diagonal"]))
        with np.errstate(over="ignore"):                           # (a denormal radius: the quotient is inf and the solve fails, DENORMAL_RADIUS)
            D = np.sqrt(diag / radius)
        A = H.copy()
        A[:, np.arange(6), np.arange(6)] += D * D
        y = block_tridiagonal_solve(A, Cc, b, S.segments)
        ok = y is not None and np.isfinite(y).all()
        mcc = T(0)
        if ok:
            step = -y
            ms = np.zeros((len(S.act), 6), dt)
            mi, mj = S.ki >= 0, S.kj >= 0
            ms[mi] += np.einsum("nqc,nc->nq", J0[mi] * scale[S.ki[mi]][:, None, :], step[S.ki[mi]])
            ms[mj] += np.einsum("nqc,nc->nq", J1[mj] * scale[S.kj[mj]][:, None, :], step[S.kj[mj]])
            mcc = -(ms * (r + ms / T(2))).sum()
        if not (ok and mcc > 0):
            dec += "i"
            num_invalid += 1
            if num_invalid >= o["max_consecutive_invalid_steps"]:
                term = TERM_INVALID_STEPS if ok else TERM_FAILURE; dec += "x"; break
            radius, df = lm_step_rejected(radius, df)
            cur["cost"] = f(x_cost)
            continue
        num_invalid = 0
        cur["step_is_valid"] = 1
        cand = x.copy()
        cand[pp] = plus(x[pp], (step * scale)[prog])
        rc, _, _ = residuals(S, cand, False)
        cand_cost = T(0.5) * (rc * rc).sum()
        step_sq = ((x[pp] - cand[pp]) ** 2).sum()
        cur["step_norm"] = f(np.sqrt(step_sq)); cur["cost_change"] = f(x_cost - cand_cost)
        if np.sqrt(step_sq) <= o["parameter_tolerance"] * (x_norm + o["parameter_tolerance"]):
            term = TERM_PARAMETER_TOL; dec += "p"; break
        if abs(x_cost - cand_cost) <= o["function_tolerance"] * x_cost:
            term = TERM_FUNCTION_TOL; dec += "f"; break
        rel = max((ev_cur - cand_cost) / mcc, (ev_ref - cand_cost) / (ev_acc_ref + mcc))
        cur["relative_decrease"] = f(rel)
        if rel > o["min_relative_decrease"]:
            dec += "o"
            x = cand
            x_norm = np.sqrt((x[pp] ** 2).sum())
            r, J0, J1 = residuals(S, x)
            x_cost = T(0.5) * (r * r).sum()
            H, Cc, b, g = assemble(S, J0, J1, r, scale)
            gmax = np.abs(g[prog]).max()
            step_successful = True
            cur["step_is_successful"] = 1; cur["cost"] = f(x_cost); cur["gradient_max_norm"] = f(gmax)
            radius, df = lm_step_accepted(radius, rel, T(o["max_radius"]))
            radius, df = T(radius), T(df)
            ev_cur = cand_cost; ev_acc_cand += mcc; ev_acc_ref += mcc
            if ev_cur < ev_min:
                ev_min = ev_cur; ev_nonmono = 0; ev_cand = ev_cur; ev_acc_cand = T(0)
            else:
                ev_nonmono += 1
                if ev_cur > ev_cand:
                    ev_cand = ev_cur; ev_acc_cand = T(0)
            if ev_nonmono == 0:
                ev_ref = ev_cand; ev_acc_ref = ev_acc_cand
        else:
            dec += "r"
            radius, df = lm_step_rejected(radius, df)
            cur["cost"] = f(cand_cost)
    out = x if term != TERM_FAILURE else np.asarray(prob["poses"], np.float64).reshape(-1, 7).astype(dt)
    return dict(poses=out, iterations=n_steps, num_successful_steps=n_success, initial_cost=initial_cost, final_cost=minimum_cost,
                termination=term, trace=trace, decisions=dec)


# ----------------------------------------------------------------------------------------------------------- after the solve
def apply(win_old, win_new, ini_Tcw, newopt_Twc, young_old, xyz, pt_kf, dt=np.float64):
    """src/optimizer.cpp:2476-2585: young_new = newopt_Twc (ini_Tcw young_old); xyz' = Twc_new (Tcw_old xyz) with the keyframe the
    point is anchored in (window keyframes first, then the younger ones).  -> (young_new (n, 7), xyz_out (m, 3))"""
    wo = np.asarray(win_old, dt).reshape(-1, 7); wn = np.asarray(win_new, dt).reshape(-1, 7)
    yo = np.asarray(young_old, dt).reshape(-1, 7); X = np.asarray(xyz, dt).reshape(-1, 3); kf = np.asarray(pt_kf, np.int64)
    ny = len(yo)
    one = lambda T: tuple(np.repeat(a, ny, axis=0) for a in load(np.asarray(T, dt).reshape(1, 7), dt))
    yn = store(mul(one(newopt_Twc), mul(one(ini_Tcw), load(yo, dt)))) if ny else np.zeros((0, 7), dt)
    old = np.concatenate([wo, yo]); new = np.concatenate([wn, yn])
    if not len(X):
        return yn, np.zeros((0, 3), dt)
    Tcw = inv(load(old[kf], dt)); Tn = load(new[kf], dt)
    cam = rot(Tcw[0], X) + Tcw[1]
    return yn, rot(Tn[0], cam) + Tn[1]


# ----------------------------------------------------------------------------------------------------------- scenes
def _exp_pose(rng, sig_t, sig_r, n):
    """n small random motions [t q] (float64)"""
    d = np.concatenate([rng.normal(0, sig_t, (n, 3)), rng.normal(0, sig_r, (n, 3))], axis=1)
    I = np.tile(np.array([0, 0, 0, 0, 0, 0, 1.0]), (n, 1))
    return plus(I, d)


def arc(n, radius=20.0, turn=1.5 * np.pi):
    """ground truth: n poses on a smooth arc, camera looking along the tangent"""
    a = np.linspace(0.0, turn, n) if n > 1 else np.zeros(1)
    P = np.zeros((n, 7))
    P[:, 0] = radius * np.sin(a); P[:, 1] = radius * (1 - np.cos(a)); P[:, 2] = 0.3 * np.sin(3 * a)
    P[:, 5] = np.sin(a / 2); P[:, 6] = np.cos(a / 2)
    return P


def make_local_scene(rng, n, loop_t=0.005, loop_r=0.001, loop_far=False):
    """localPoseGraph after a loop closure over n keyframes: odometry with N(0, 1 cm) / N(0, 2 mrad) noise per step integrated into
    the initial estimate, chain measurements taken from that estimate (src/optimizer.cpp:2411), the loop measurement from ground
    truth plus N(0, loop_t) / N(0, loop_r).  loop_far: displaced by N(0, 30 m) and rotated by 3.0-3.14 rad instead (a wrong loop:
    steps get rejected)."""
    gt = arc(n)
    est = np.zeros((n, 7)); est[0] = gt[0]
    noise = _exp_pose(rng, 0.01, 0.002, n)
    for k in range(1, n):
        rel = mul_pose(inv_pose(gt[k - 1]), gt[k])
        est[k] = mul_pose(est[k - 1], mul_pose(rel, noise[k]))
    loop = mul_pose(inv_pose(gt[0]), gt[n - 1])
    if loop_far:
        ax = rng.normal(0, 1, 3); ax /= np.linalg.norm(ax)
        ang = rng.uniform(3.0, 3.14)
        d = np.concatenate([rng.normal(0, 30.0, 3), np.sin(ang / 2) * ax, [np.cos(ang / 2)]])
        loop = mul_pose(loop, d)
    else:
        loop = mul_pose(loop, _exp_pose(rng, loop_t, loop_r, 1)[0])
    return local_pose_graph(list(est), loop)


def make_full_scene(rng, n, every, extra_kf=(), open_end=False):
    """fullPoseGraph: n frames, a keyframe every `every` frames (plus the ids in extra_kf; open_end: none after the last regular one,
    so the trajectory ends in variable frames when (n - 1) % every != 0).  The keyframes carry the corrected (ground-truth) poses,
    the other frames the drifting odometry estimate, vTpc the odometry's relative poses."""
    gt = arc(n, radius=15.0, turn=np.pi)
    noise = _exp_pose(rng, 0.01, 0.002, n)
    est = np.zeros((n, 7)); est[0] = gt[0]
    vTpc = np.tile(np.array([0, 0, 0, 0, 0, 0, 1.0]), (n, 1))
    for k in range(1, n):
        vTpc[k] = mul_pose(mul_pose(inv_pose(gt[k - 1]), gt[k]), noise[k])
        est[k] = mul_pose(est[k - 1], vTpc[k])
    iskf = np.zeros(n, bool); iskf[::every] = True
    for k in extra_kf:
        iskf[k] = True
    if not open_end:
        iskf[n - 1] = True
    vTwc = np.where(iskf[:, None], gt, est)
    return full_pose_graph(vTwc, vTpc, iskf)


def reverse_edges(prob):
    """the same problem with every edge turned round: (j, i) measuring Tc_j c_i = (Tc_i c_j)^-1"""
    p = dict(prob)
    p["edge_i"], p["edge_j"] = np.asarray(prob["edge_j"]).copy(), np.asarray(prob["edge_i"]).copy()
    p["edge_T"] = store(inv(load(prob["edge_T"])))
    return p
