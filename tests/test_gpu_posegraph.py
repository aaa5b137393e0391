"""The device pose-graph solver (csrc/posegraph.hip: ov2_pose_graph_solve[_batch], ov2_pose_graph_apply) against the numpy
specification (tests/posegraph_ref.py, pinned to the reference's factor by tests/test_posegraph_reference.py).

DECISIONS are compared exactly with the float64 specification: iterations, successful steps, termination and the trace's
step_is_valid / step_is_successful per iteration.  CONDITION: the float64 and the longdouble specification make the same decisions
on every committed case (asserted; another seed otherwise).

NUMBERS: every pose component must lie within

    max(1e-12 max(1, |pose|), 100 x max |float64 - longdouble| of the specification's poses on that case)

and the trace's cost and trust-region radius are held to the same rule at every iteration: entry v of a field within
max(1e-12 max(1, |v|), 100 x |v| x the largest relative float64 - longdouble difference of that field over the case's trace).  The
difference of the case, not of the single entry: along a rejecting sequence the two precisions cross, so a single entry can agree
to 1e-14 next to entries that differ by 1e-11, and says nothing about how far another operation order may move it.  The bound follows the case's conditioning: the two precisions differ by 1.5e-15 at N = 2 and by 4e-10 at N = 1500.  100 x is for
another order of the same operations, the convention of tests/test_gpu_fivept.py.

INDEPENDENT OF CONDITIONING: the specification's cost at the device's poses_out equals the device's final_cost to 1e-12 relative
(plus 3 n_edges (4 eps max|t|)^2, the cost of residuals that are nothing but the rounding of the pose products: it decides at the
optimum only, where the cost is 1e-28), and

    final_cost(device) <= final_cost(spec) + |g|_1 tol + 1e-12 final_cost(spec),

g the specification's gradient J^T r (tangent space, all variable poses) at its own final poses and tol the pose bound above: the
first-order change of the cost over a box of half-width tol around the specification's solution.

OV2_TERM_FAILURE: no finite POSE or MEASUREMENT gives a failed factorisation -- the factor's Jacobian blocks (I -+ J_c / 2) Adj(.)
are never singular (the eigenvalues of I -+ hat(omega) / 2 are 1 and 1 -+ i theta / 2) and min_lm_diagonal > 0 is added on top -- but
a finite, accepted initial_radius does: at 1e-310 diag / radius overflows, every pivot is inf and every step invalid
(posegraph_ref.DENORMAL_RADIUS).  On that case the longdouble specification does not overflow, so the condition above does not
apply to it and only decisions and copied values are compared: iterations, termination, the trace's flags and radii (halving a
double is exact), poses_out equal to the input bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from tests import posegraph_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOCAL_NS = (2, 3, 5, 63, 64, 65, 130, 257, 513, 1500)       # 63 / 64 / 65: one wavefront of edges and its neighbours; 257 / 513: one and two
FAR_NS = (3, 9, 17)                                        # work-group strides; 1500: one long segment
FULL = {"30_5": (30, 5, (), False), "130_7": (130, 7, (), False), "257_11": (257, 11, (), False),
        "130_7_twokf": (130, 7, (50,), False),              # frames 49 and 50 are both keyframes: a constant-constant edge
        "130_7_open": (130, 7, (), True)}                   # the last frames are not followed by a keyframe
FLOOR = 1e-12

_cache = {}
_worst = {"ratio": 0.0}


def _problem(kind, key):
    if kind == "local":
        return R.make_local_scene(np.random.default_rng(100 + key), key), False
    if kind == "far":
        return R.make_local_scene(np.random.default_rng(7 + key), key, loop_far=True), False
    if kind == "full":
        n, every, extra, open_end = FULL[key]
        return R.make_full_scene(np.random.default_rng(n), n, every, extra, open_end), True
    if kind == "reversed":
        return R.reverse_edges(_problem("local", key)[0]), False
    if kind == "optimum":                                    # every measurement agrees with the poses: the gradient vanishes at the start
        p = R.make_local_scene(np.random.default_rng(5), key)
        p["edge_T"][-1] = R.mul_pose(R.inv_pose(p["poses"][0]), p["poses"][-1])
        return p, False
    raise KeyError(kind)


def case(kind, key, **opt):
    """the committed case, with the specification's solve in float64 and in longdouble (computed once per module)"""
    k = (kind, key, tuple(sorted(opt.items())))
    if k not in _cache:
        prob, full = _problem(kind, key)
        o = R.options(full=full, **opt)
        a, b = R.solve(prob, o), R.solve(prob, o, np.longdouble)
        assert a["decisions"] == b["decisions"] and a["termination"] == b["termination"] and a["iterations"] == b["iterations"], \
            "float64 and longdouble decide differently on this case: choose another seed"
        _cache[k] = dict(prob=prob, full=full, opt=opt, want=a, want_ld=b, spread=float(np.abs(a["poses"] - b["poses"]).max()))
    return _cache[k]


def _options(ctx, c):
    from ov2slam_amd import optimizer as O
    names = dict(max_iter="max_iter")
    return O.pose_graph_options(ctx.lib, full=c["full"], **{names[k]: v for k, v in c["opt"].items()})


def _tol(c, ref):
    return np.maximum(FLOOR * np.maximum(1.0, np.abs(ref)), 100.0 * c["spread"])


def _compare(c, got, trace=True):
    want, ld = c["want"], c["want_ld"]
    print("spec: %s, %d iterations, termination %d, cost %.6g -> %.6g, float64 - longdouble %.3g" %
          (want["decisions"], want["iterations"], want["termination"], want["initial_cost"], want["final_cost"], c["spread"]))
    print("device: %d iterations, %d successful, termination %d, cost %.17g -> %.17g, %.3f ms" %
          (got["iterations"], got["num_successful_steps"], got["termination"], got["initial_cost"], got["final_cost"], got["solve_ms"]))
    assert got["iterations"] == want["iterations"] and got["num_successful_steps"] == want["num_successful_steps"]
    assert got["termination"] == want["termination"]
    d = np.abs(got["poses"] - want["poses"])
    tol = _tol(c, want["poses"])
    ratio = float((d / tol).max())
    _worst["ratio"] = max(_worst["ratio"], ratio)
    print("poses: largest difference %.3g, %.3g of its bound; worst ratio of the module so far %.3g" % (d.max(), ratio, _worst["ratio"]))
    assert (d <= tol).all()
    if trace:
        tr, wt, lt = got["trace"], want["trace"], ld["trace"]
        assert len(tr) == len(wt)
        rel = {f: max([abs(w[f] - l[f]) / abs(w[f]) for w, l in zip(wt, lt) if w[f] != 0.0] or [0.0]) for f in ("cost", "trust_region_radius")}
        for g, w, l in zip(tr, wt, lt):
            assert (g["iteration"], g["step_is_valid"], g["step_is_successful"]) == (w["iteration"], w["step_is_valid"], w["step_is_successful"])
            for f in ("cost", "trust_region_radius"):
                bound = max(FLOOR * max(1.0, abs(w[f])), 100.0 * rel[f] * abs(w[f]))
                r = abs(g[f] - w[f]) / bound
                _worst["ratio"] = max(_worst["ratio"], r)
                print("  it %d %s: device %.17g spec %.17g, %.3g of its bound" % (g["iteration"], f, g[f], w[f], r))
                assert abs(g[f] - w[f]) <= bound, (g["iteration"], f, g[f], w[f], bound)
    if want["iterations"] or want["trace"]:
        at = float(R.cost(c["prob"], got["poses"]))
        print("spec cost at the device's poses %.17g, device final_cost %.17g, relative difference %.3g" %
              (at, got["final_cost"], abs(at - got["final_cost"]) / max(at, 1e-300)))
        noise = 3.0 * len(c["prob"]["edge_i"]) * (4.0 * np.finfo(np.float64).eps * float(np.abs(c["prob"]["poses"][:, :3]).max())) ** 2
        assert abs(at - got["final_cost"]) <= 1e-12 * at + noise
        g1 = float(np.abs(R.gradient(c["prob"], want["poses"])).sum())
        wf = float(want["final_cost"])
        print("final cost: device - spec %.3g, allowed %.3g" % (got["final_cost"] - wf, g1 * float(tol.max()) + 1e-12 * wf))
        assert got["final_cost"] <= wf + g1 * float(tol.max()) + 1e-12 * wf


def _solve(ctx, c, trace=True):
    from ov2slam_amd import optimizer as O
    return O.pose_graph(ctx, c["prob"], _options(ctx, c), trace=trace)


@pytest.mark.gpu
@pytest.mark.parametrize("n", LOCAL_NS)
def test_local_pose_graph(gpu_ctx, n):
    c = case("local", n)
    _compare(c, _solve(gpu_ctx, c))
    assert np.array_equal(_solve(gpu_ctx, c)["poses"][0], c["prob"]["poses"][0])         # the loop keyframe is constant


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(FULL))
def test_full_pose_graph(gpu_ctx, key):
    c = case("full", key)
    got = _solve(gpu_ctx, c)
    _compare(c, got)
    kf = c["prob"]["pose_const"].astype(bool)
    assert np.array_equal(got["poses"][kf], c["prob"]["poses"][kf])
    if key == "130_7_twokf":
        assert kf[49] and kf[50]
    if key == "130_7_open":
        assert not kf[-1]


@pytest.mark.gpu
@pytest.mark.parametrize("n", FAR_NS)
def test_rejected_steps(gpu_ctx, n):
    """a wrong loop measurement (30 m, about pi away): the specification rejects steps, and so must the device, at the same places"""
    c = case("far", n)
    assert "r" in c["want"]["decisions"]
    _compare(c, _solve(gpu_ctx, c))


@pytest.mark.gpu
def test_at_the_optimum_the_gradient_exit_comes_at_iteration_zero(gpu_ctx):
    c = case("optimum", 9)
    assert c["want"]["termination"] == R.TERM_GRADIENT_TOL and c["want"]["iterations"] == 0
    got = _solve(gpu_ctx, c)
    _compare(c, got)
    assert got["iterations"] == 0 and got["termination"] == R.TERM_GRADIENT_TOL and np.array_equal(got["poses"], c["prob"]["poses"])


@pytest.mark.gpu
def test_max_iter_zero(gpu_ctx):
    c = case("local", 17, max_iter=0)
    got = _solve(gpu_ctx, c)
    _compare(c, got)
    assert got["iterations"] == 0 and got["termination"] == R.TERM_NO_CONVERGENCE and np.array_equal(got["poses"], c["prob"]["poses"])
    assert got["initial_cost"] == got["final_cost"] > 0


@pytest.mark.gpu
def test_nothing_to_optimise(gpu_ctx):
    """no variable pose, or no edge that touches one: OV2_OK, the input poses, 0 iterations, FUNCTION_TOLERANCE"""
    from ov2slam_amd import optimizer as O
    p = dict(case("local", 5)["prob"])
    allc = dict(p, pose_const=np.ones(5, np.uint8))
    noedge = dict(p, edge_i=np.zeros(0, np.int32), edge_j=np.zeros(0, np.int32), edge_T=np.zeros((0, 7)))
    cc_only = dict(p, pose_const=np.array([1, 1, 0, 0, 0], np.uint8), edge_i=np.array([0], np.int32), edge_j=np.array([1], np.int32),
                   edge_T=p["edge_T"][:1])
    for q in (allc, noedge, cc_only):
        got = O.pose_graph(gpu_ctx, q)
        assert got["iterations"] == 0 and got["termination"] == R.TERM_FUNCTION_TOL and np.array_equal(got["poses"], p["poses"])
        assert got["initial_cost"] == 0.0 and got["final_cost"] == 0.0


@pytest.mark.gpu
def test_reversed_edges(gpu_ctx):
    """every edge turned round, (j, i) with the inverted measurement: the device must solve THAT problem as the specification
    does (same bound) -- an edge may point backwards along the chain"""
    c = case("reversed", 65)
    assert (c["prob"]["edge_i"][:-1] > c["prob"]["edge_j"][:-1]).all()
    _compare(c, _solve(gpu_ctx, c))


@pytest.mark.gpu
def test_batch_returns_the_bytes_of_the_single_calls(gpu_ctx):
    from ov2slam_amd import optimizer as O
    cases = [case("local", n) for n in LOCAL_NS if n <= 513] + [case("far", n) for n in FAR_NS]
    order = np.random.default_rng(3).permutation(len(cases))
    opts = O.pose_graph_options(gpu_ctx.lib)
    singles = [O.pose_graph(gpu_ctx, cases[i]["prob"], opts) for i in order]
    probs = [cases[i]["prob"] for i in order]
    a = O.pose_graph_batch(gpu_ctx, probs, opts)
    b = O.pose_graph_batch(gpu_ctx, probs, opts)
    for s, x, y in zip(singles, a, b):
        for f in ("iterations", "num_successful_steps", "termination", "initial_cost", "final_cost"):
            assert s[f] == x[f] == y[f], f
        assert s["poses"].tobytes() == x["poses"].tobytes() == y["poses"].tobytes()
    # items with nothing to solve beside one that is solved: no pose at all, one pose (no edge can touch it), 17 poses
    one = case("far", 17)["prob"]
    none = dict(poses=np.zeros((0, 7)), pose_const=np.zeros(0, np.uint8), edge_i=np.zeros(0, np.int32), edge_j=np.zeros(0, np.int32),
                edge_T=np.zeros((0, 7)))
    lone = dict(none, poses=one["poses"][:1], pose_const=np.zeros(1, np.uint8))
    for probs in ([none, lone, one], [one, none]):
        for p, x in zip(probs, O.pose_graph_batch(gpu_ctx, probs, opts)):
            s = O.pose_graph(gpu_ctx, p, opts)
            for f in ("iterations", "num_successful_steps", "termination", "initial_cost", "final_cost"):
                assert s[f] == x[f], f
            assert s["poses"].tobytes() == x["poses"].tobytes() and len(x["poses"]) == len(p["poses"])
            if p is not one:
                assert x["iterations"] == 0 and x["termination"] == R.TERM_FUNCTION_TOL and np.array_equal(x["poses"], p["poses"])
    assert O.pose_graph_batch(gpu_ctx, [], opts) == []


DENORMAL_VARIANTS = {"five_invalid": (dict(), "iiiiix", R.TERM_FAILURE, 5),
                     "budget2": (dict(max_consecutive_invalid_steps=2), "iix", R.TERM_FAILURE, 2),
                     "min_radius_after_invalid": (dict(min_radius=1e-312), "iiiis", R.TERM_MIN_RADIUS, 4)}


def _denormal(ctx, variant, trace=True):
    """-> (problem, the float64 specification's solve, the device's) under posegraph_ref.DENORMAL_RADIUS"""
    from ov2slam_amd import optimizer as O
    kw = dict(R.DENORMAL_RADIUS, **DENORMAL_VARIANTS[variant][0])
    p = R.denormal_radius_scene()
    return p, R.solve(p, R.options(**kw)), O.pose_graph(ctx, p, O.pose_graph_options(ctx.lib, **kw), trace=trace)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", sorted(DENORMAL_VARIANTS))
def test_denormal_radius_fails_every_solve(gpu_ctx, variant):
    """every linear solve fails: OV2_TERM_FAILURE (the radius floor, where it comes first: MIN_RADIUS) and the input poses"""
    _, dec, term, its = DENORMAL_VARIANTS[variant]
    p, want, got = _denormal(gpu_ctx, variant)
    assert (want["decisions"], want["termination"], want["iterations"]) == (dec, term, its)
    assert (got["iterations"], got["num_successful_steps"], got["termination"]) == (its, 1, term)
    assert got["poses"].tobytes() == np.ascontiguousarray(p["poses"], np.float64).tobytes()
    assert got["initial_cost"] == got["final_cost"] and abs(got["initial_cost"] - want["initial_cost"]) <= 1e-12 * want["initial_cost"]
    flags = lambda tr: [(t["iteration"], t["step_is_valid"], t["step_is_successful"], t["trust_region_radius"]) for t in tr]
    assert flags(got["trace"]) == flags(want["trace"]) and len(got["trace"]) == dec.count("i") + (term == R.TERM_MIN_RADIUS)
    assert all(t["cost"] == got["initial_cost"] and t["cost_change"] == 0 and t["step_norm"] == 0 for t in got["trace"][1:])


@pytest.mark.gpu
def test_failing_item_in_a_batch_leaves_its_neighbours_alone(gpu_ctx):
    """A batch has ONE option set, and with Jacobi scaling the LM diagonal lies in [min_lm_diagonal, 1): what fails under a radius
    is decided by the problem's weights.  At initial_radius 5e-312 diag / radius overflows from diag = 9e-4 on: the denormal-radius
    scene (sigma 1, diag near 1) fails every solve, two scenes whose edges weigh 1e-4 (diag <= 1e-5) do not -- their one step is
    lost in rounding and the function tolerance ends them, as in the specification.  The batch [scene, failing, scene] returns the
    bytes of the three single calls, the failing item its input poses."""
    from ov2slam_amd import optimizer as O
    kw = dict(R.DENORMAL_RADIUS, initial_radius=5e-312)
    opts = O.pose_graph_options(gpu_ctx.lib, **kw)
    weak = lambda q: dict(q, edge_sigma=np.full(len(q["edge_i"]), 1e4))
    bad = R.denormal_radius_scene()
    a, c = weak(case("local", 17)["prob"]), weak(case("far", 9)["prob"])
    probs = [a, bad, c]
    spec = [R.solve(q, R.options(**kw)) for q in probs]
    assert [s["decisions"] for s in spec] == ["f", "iiiiix", "f"] and spec[1]["termination"] == R.TERM_FAILURE
    singles = [O.pose_graph(gpu_ctx, q, opts) for q in probs]
    batch = O.pose_graph_batch(gpu_ctx, probs, opts)
    for q, w, s, x in zip(probs, spec, singles, batch):
        for f in ("iterations", "num_successful_steps", "termination", "initial_cost", "final_cost"):
            assert s[f] == x[f], f
        assert s["poses"].tobytes() == x["poses"].tobytes()
        assert (x["iterations"], x["num_successful_steps"], x["termination"]) == (w["iterations"], w["num_successful_steps"], w["termination"])
        assert x["poses"].tobytes() == np.ascontiguousarray(q["poses"], np.float64).tobytes()       # (no step is taken in any of them)
    assert batch[1]["termination"] == R.TERM_FAILURE and batch[0]["termination"] == batch[2]["termination"] == R.TERM_FUNCTION_TOL
    # and beside items that do move: the failing scene under ordinary options is an ordinary item again
    moving = O.pose_graph_batch(gpu_ctx, [case("local", 17)["prob"], bad, case("far", 9)["prob"]], O.pose_graph_options(gpu_ctx.lib))
    assert all(m["termination"] != R.TERM_FAILURE and m["final_cost"] < m["initial_cost"] for m in moving)


@pytest.mark.gpu
def test_two_runs_return_the_same_bytes(gpu_ctx):
    c = case("full", "257_11")
    a, b = _solve(gpu_ctx, c), _solve(gpu_ctx, c)
    assert a["poses"].tobytes() == b["poses"].tobytes() and a["final_cost"] == b["final_cost"]
    key = lambda t: tuple(sorted((k, v) for k, v in t.items() if k != "gradient_norm"))      # (gradient_norm is NaN: the device forms the max norm only)
    assert [key(t) for t in a["trace"]] == [key(t) for t in b["trace"]]


@pytest.mark.gpu
def test_optimizer_methods_build_and_solve_the_reference_problems(gpu_ctx):
    """Optimizer.localPoseGraph / fullPoseGraph: the builders' problems under the reference's two option sets"""
    from ov2slam_amd import optimizer as O
    opt = O.Optimizer(gpu_ctx)
    c = case("local", 65)
    got = opt.localPoseGraph(list(c["prob"]["poses"]), c["prob"]["edge_T"][-1])
    _compare(c, dict(got, trace=[]), trace=False)
    cf = case("full", "130_7")
    p = cf["prob"]
    vTpc = np.concatenate([[[0, 0, 0, 0, 0, 0, 1.0]], p["edge_T"]])
    _compare(cf, dict(opt.fullPoseGraph(p["poses"], vTpc, p["pose_const"]), trace=[]), trace=False)


def _apply_case(n_win=21, n_young=5, n_pts=3000):
    rng = np.random.default_rng(11)
    P = R.arc(n_win + n_young + 1)
    new = R.plus(P.copy(), np.concatenate([rng.normal(0, 0.05, (len(P), 3)), rng.normal(0, 0.01, (len(P), 3))], axis=1))
    win_old, win_new, young_old = P[:n_win], new[:n_win], P[n_win:n_win + n_young]
    ini_Tcw, newopt = R.inv_pose(P[n_win - 1]), new[n_win - 1]
    kf = rng.integers(0, max(1, n_win + n_young), n_pts).astype(np.int32)
    xyz = np.concatenate([P[:n_win + n_young][kf, :3] + rng.normal(0, 5.0, (n_pts, 3))]) if n_pts else np.zeros((0, 3))
    return win_old, win_new, ini_Tcw, newopt, young_old, xyz, kf


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(21, 5, 3000), (21, 0, 3000), (21, 5, 0)], ids=["full", "no_young", "no_points"])
def test_apply(gpu_ctx, shape):
    from ov2slam_amd import optimizer as O
    args = _apply_case(*shape)
    yn, X = O.pose_graph_apply(gpu_ctx, *args)
    wy, wX = R.apply(*args)
    ly, lX = R.apply(*args, dt=np.longdouble)
    assert yn.shape == (shape[1], 7) and X.shape == (shape[2], 3)
    for g, w, l in ((yn, wy, ly), (X, wX, lX)):
        if g.size:
            spread = float(np.abs(w - l).max())
            tol = np.maximum(FLOOR * np.maximum(1.0, np.abs(w)), 100.0 * spread)
            print("apply: largest difference %.3g, %.3g of its bound" % (np.abs(g - w).max(), (np.abs(g - w) / tol).max()))
            assert (np.abs(g - w) <= tol).all()


def _wr(f, a):
    a = np.ascontiguousarray(a)
    f.write(np.int64(a.nbytes).tobytes()); f.write(a.tobytes())


def _rd(f, dt):
    nb = int(np.frombuffer(f.read(8), np.int64)[0])
    return np.frombuffer(f.read(nb), dt)


@pytest.mark.gpu
def test_cpp_adapter(gpu_ctx, tmp_path):
    """tests/cpp/posegraph_run.cpp: ov2::Optimizer::solvePoseGraph on a FlatPoseGraph returns the bytes of the Python path"""
    exe = tmp_path / "posegraph_run"
    libdir = os.path.join(ROOT, "ov2slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "posegraph_run.cpp"),
                           "-o", str(exe), "-L", libdir, "-lov2slam_hip", "-Wl,-rpath," + libdir])
    c = case("local", 65)
    p = c["prob"]
    cf, rf = tmp_path / "case.bin", tmp_path / "res.bin"
    with open(cf, "wb") as f:
        _wr(f, p["poses"]); _wr(f, p["pose_const"]); _wr(f, p["edge_i"]); _wr(f, p["edge_j"]); _wr(f, p["edge_T"]); _wr(f, np.array([0], np.int32))
    r = subprocess.run([str(exe), str(cf), str(rf)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    py = _solve(gpu_ctx, c, trace=False)
    with open(rf, "rb") as f:
        ok, term, out = _rd(f, np.int32), _rd(f, np.int32), _rd(f, np.float64)
    assert ok[0] == 1 and term[0] == py["termination"]
    assert out.tobytes() == py["poses"].tobytes()


@pytest.mark.gpu
def test_worst_ratio_is_reported():
    """after the cases above (shared state): the figure DESIGN.md 4.12 quotes"""
    print("worst device - specification difference of the module: %.3g of its bound" % _worst["ratio"])
    assert _worst["ratio"] <= 1.0
