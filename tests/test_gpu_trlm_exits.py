"""The device solvers on tests/trlm_cases.py against the oracle: invalid steps (a failed or non-finite linear solve, HandleInvalidStep
in csrc/ba_core.hpp), the recovery from them, and every exit of the trust-region loop -- NO_CONVERGENCE, FUNCTION_TOL, PARAMETER_TOL,
GRADIENT_TOL, MIN_RADIUS, INVALID_STEPS -- on
  * ov2_ba_solve on each path of tests/test_gpu_ba_structure.py's PATHS, with the trace,
  * ov2_ba_solve on the one-pose problem, which runs the one-kernel pose-only solver (k_ba_pose_only), with the trace,
  * ov2_xyz_ba_solve and ov2_structure_ba (no trace on either side: counts and exit).
Decisions are identical: iterations, termination, successful steps, the S / r / i pattern; the radii of the trace are equal bit for
bit (halving and tripling a double is exact or correctly rounded on both sides).  A solve that never takes a step returns its inputs
bit for bit with final_cost == initial_cost, and where it never evaluates a step either its chi2 and depth flags are those of a
max_iter = 0 device solve.  Solves that move are held to the bars already in force: _cmp of tests/test_gpu_ba.py (tests/test_gpu_xyz_ba.py
for the point form), the structure-only bar of tests/test_gpu_ba_structure.py, and same_solve at the 1e-8 of
test_device_trace_agrees_with_ceres_own_loop.

Not here: pnp.hip keeps its own copy of the loop with fixed options (ceresPnP's) and cannot be steered to these cases."""
import numpy as np
import pytest

from ov2slam_amd import optimizer
from tests import trlm_cases as TC
from tests.test_gpu_ba import _cmp
from tests.test_gpu_ba_structure import PATHS
from tests.test_gpu_xyz_ba import _cmp as _cmp_xyz
from tests.test_reference_trlm import same_solve

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solved(oracle):
    """name -> (problem, the oracle's result), each case solved once"""
    pbs = {k: f() for k, f in TC.PROBLEMS.items()}
    return {c.name: (pbs[c.problem], TC.oracle_solve(oracle, c, pbs[c.problem])) for c in TC.CASES}


def _device(ctx, case, pb, **override):
    opts = optimizer.default_options(ctx.lib, **dict(case.options, **override))
    if case.solver == "ba":
        return optimizer.solve(ctx, pb, opts, trace=True)
    return (optimizer.solve_xyz if case.solver == "xyz" else optimizer.structure_only_ba)(ctx, pb, opts)


def _cmp_struct(g, r):
    assert abs(g["initial_cost"] - r["initial_cost"]) <= 1e-10 * abs(r["initial_cost"])
    assert abs(g["final_cost"] - r["final_cost"]) <= 1e-8 * abs(r["final_cost"])
    assert np.abs(g["xyz"] - r["xyz"]).max() <= 1e-7 * max(1.0, np.abs(r["xyz"]).max())
    assert np.allclose(g["chi2"], r["chi2"], rtol=1e-6, atol=1e-9) and np.array_equal(g["depthpos"], r["depthpos"])


def _check(ctx, case, pb, r):
    g = _device(ctx, case, pb)
    pat = TC.pattern(g["trace"]) if "trace" in g else None
    assert (g["iterations"], g["termination"], g["num_successful_steps"], pat) == (case.iterations, case.termination, case.successful, case.pattern), \
        (case.name, g["iterations"], g["termination"], g["num_successful_steps"], pat)
    assert (r["iterations"], r["termination"], r["num_successful_steps"]) == (case.iterations, case.termination, case.successful)
    if pat is not None:
        assert [t["trust_region_radius"] for t in g["trace"]] == [t["trust_region_radius"] for t in r["trace"]]
        same_solve(g, r, 1e-8, case.name, gradient_norm=False)
    if case.kind in ("all_invalid", "unchanged"):
        assert TC.inputs_returned(case, pb, g), case.name
        assert g["final_cost"] == g["initial_cost"]
    if case.kind == "all_invalid":
        # the last evaluated point is the initial one
        z = _device(ctx, case, pb, max_iter=0)
        # (per-block values: the cost itself is summed with atomics, in an order that varies from solve to solve)
        assert z["iterations"] == 0 and abs(z["initial_cost"] - g["initial_cost"]) <= 1e-10 * g["initial_cost"]
        assert np.array_equal(g["chi2"], z["chi2"], equal_nan=True) and np.array_equal(g["depthpos"], z["depthpos"])
    if case.solver == "ba":
        _cmp(g, r, pb)
    elif case.solver == "xyz":
        _cmp_xyz(g, r)
    else:
        _cmp_struct(g, r)
    return g


BA = [c for c in TC.CASES if c.solver == "ba" and c.problem != "pnp"]


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("case", BA, ids=lambda c: c.name)
def test_ba_solve_takes_every_exit_on_every_path(gpu_ctx, solved, case, path):
    with gpu_ctx.options(**PATHS[path]):
        g = _check(gpu_ctx, case, *solved[case.name])
        if path == "deterministic":
            g2 = _device(gpu_ctx, case, solved[case.name][0])
            for k in ("poses", "invdepth", "chi2", "depthpos"):
                assert np.array_equal(g2[k], g[k], equal_nan=True), k
    if case.problem == "irregular":
        # the free keyframe without blocks, whose pivot makes the steps invalid, never moves
        pb = solved[case.name][0]
        assert np.array_equal(g["poses"][pb["empty_kf"]], pb["poses"][pb["empty_kf"]])


def test_every_exit_code_is_reached_by_ba_solve():
    assert {c.termination for c in BA} == set(range(6))
    assert any("iSi" in c.pattern for c in BA)


@pytest.mark.parametrize("case", [c for c in TC.CASES if c.problem == "pnp"], ids=lambda c: c.name)
def test_pose_only_solver_takes_every_exit(gpu_ctx, solved, case):
    _check(gpu_ctx, case, *solved[case.name])


@pytest.mark.parametrize("case", [c for c in TC.CASES if c.solver == "xyz"], ids=lambda c: c.name)
def test_xyz_solver_takes_every_exit(gpu_ctx, solved, case):
    pb, r = solved[case.name]
    for opts in (dict(), dict(ba_force_large=1)):
        with gpu_ctx.options(**opts):
            g = _check(gpu_ctx, case, pb, r)
    if case.problem == "recovery_xyz":
        assert np.array_equal(g["poses"][pb["empty_kf"]], pb["poses"][pb["empty_kf"]])


@pytest.mark.parametrize("case", [c for c in TC.CASES if c.solver == "struct"], ids=lambda c: c.name)
def test_structure_only_solver_takes_every_exit(gpu_ctx, solved, case):
    _check(gpu_ctx, case, *solved[case.name])


def test_the_other_solvers_reach_the_exits_too():
    want = {TC.TERM[k] for k in ("INVALID_STEPS", "MIN_RADIUS", "NO_CONVERGENCE", "PARAMETER_TOL", "GRADIENT_TOL")}
    for sel in (lambda c: c.problem == "pnp", lambda c: c.solver == "xyz", lambda c: c.solver == "struct"):
        assert want <= {c.termination for c in TC.CASES if sel(c)}
