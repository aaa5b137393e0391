"""tests/trlm_cases.py on the CPU: every case does on the oracle what it is for (pattern, exit, counts), the recovery cases keep
their stated distance from the rounding boundary, an all-invalid solve returns its inputs bit for bit, the tolerance exits have
their margin, and Ceres' own TrustRegionMinimizer (tests/test_reference_trlm.py's library) makes the same decisions on every
ov2_ba_solve case.  Run with -s for the pattern and exit each side reaches."""
import pytest

from tests import trlm_cases as TC
from tests.test_reference_trlm import ceres, ceres_solve, same_solve      # noqa: F401 (ceres is a fixture)

NAMES = {v: k for k, v in TC.TERM.items()}


@pytest.fixture(scope="module")
def solved(oracle):
    """name -> (problem, the oracle's result), each case solved once"""
    pbs = {k: f() for k, f in TC.PROBLEMS.items()}
    return {c.name: (pbs[c.problem], TC.oracle_solve(oracle, c, pbs[c.problem])) for c in TC.CASES}


@pytest.mark.parametrize("case", TC.CASES, ids=lambda c: c.name)
def test_oracle_takes_the_exit_the_case_is_for(solved, case):
    pb, r = solved[case.name]
    pat = TC.pattern(r["trace"]) if "trace" in r else None
    print("\n  %-34s oracle: %-9s %d iterations, %s, %d successful" % (case.name, pat, r["iterations"], NAMES[r["termination"]], r["num_successful_steps"]), end="")
    assert (r["iterations"], r["termination"], r["num_successful_steps"]) == (case.iterations, case.termination, case.successful)
    assert pat == case.pattern
    if case.kind in ("all_invalid", "unchanged"):
        assert TC.inputs_returned(case, pb, r) and r["final_cost"] == r["initial_cost"]
    else:
        assert r["final_cost"] < r["initial_cost"]
    if case.kind == "all_invalid" and pat is not None:
        assert set(pat[1:]) <= {"i"}
        # halved, quartered, ...: exact or correctly rounded in binary, denormals included
        radius, factor = case.options["initial_radius"], 2.0
        for t in r["trace"]:
            assert t["trust_region_radius"] == radius
            radius, factor = radius / factor, 2.0 * factor


def test_recovery_cases_keep_their_distance_from_the_rounding_boundary(solved):
    """u = (min_lm_diagonal / radius) / 2^-1075 of every radius a linear solve ran at: below 1 / margin or above margin, and on the
    side the step's validity says.  margin = 2 except for the one case that crosses the boundary upwards (see trlm_cases)."""
    seen = 0
    for case in TC.CASES:
        if case.margin is None:
            continue
        r = solved[case.name][1]
        used = r["trace"][:r["iterations"]]                  # trace[k]'s radius is the one iteration k + 1 solved at
        u = [TC.boundary_units(case.options["min_lm_diagonal"], t["trust_region_radius"]) for t in used]
        print("\n  %-34s u = %s" % (case.name, ", ".join("%.4g" % x for x in u)), end="")
        for k, x in enumerate(u):
            assert x < 1.0 / case.margin or x > case.margin, (case.name, k, x)
            if k + 1 < len(r["trace"]):
                assert bool(r["trace"][k + 1]["step_is_valid"]) == (x > 1.0), (case.name, k, x)
        seen += 1
    assert seen >= 3
    assert TC.BY_NAME["irregular/recover_function_tol"].margin == TC.BY_NAME["irregular/budget3"].margin == 2.0
    assert "iSi" in TC.BY_NAME["irregular/recover_then_invalid"].pattern and TC.BY_NAME["irregular/recover_then_invalid"].margin > 1.7


def test_untraced_recovery_cases_share_the_radii_of_the_traced_ones():
    """the xyz solver keeps no trace on the oracle: its recovery cases run the invalid steps at initial_radius / (1, 2, 8, 64, 1024),
    the very radii (and options) the traced cases are checked at"""
    for a, b in (("recovery_xyz/recover", "irregular/recover_function_tol"), ("recovery_xyz/recover_then_invalid", "irregular/recover_then_invalid"),
                 ("recovery_xyz/budget3", "irregular/budget3")):
        ca, cb = TC.BY_NAME[a], TC.BY_NAME[b]
        for k in ("initial_radius", "max_radius", "min_lm_diagonal"):
            assert ca.options[k] == cb.options[k]
        assert ca.iterations <= cb.iterations


@pytest.mark.parametrize("case", [c for c in TC.CASES if c.tol], ids=lambda c: c.name)
def test_tolerance_exits_have_a_margin(oracle, solved, case):
    pb, r = solved[case.name]
    for f in (1.0 / TC.TOL_MARGIN, TC.TOL_MARGIN):
        o = TC.oracle_solve(oracle, case, pb, **{case.tol: case.options[case.tol] * f})
        assert (o["iterations"], o["termination"], o["num_successful_steps"]) == (r["iterations"], r["termination"], r["num_successful_steps"]), f
    if case.tol == "gradient_tolerance" and "trace" in r:
        g = [t["gradient_max_norm"] for t in r["trace"] if t["step_is_successful"]]
        assert g[-1] < case.options[case.tol] < g[-2] and abs(case.options[case.tol] / (g[-1] * g[-2]) ** 0.5 - 1) < 0.01


@pytest.mark.parametrize("case", [c for c in TC.CASES if c.solver == "ba"], ids=lambda c: c.name)
def test_ceres_own_loop_decides_alike(ceres, oracle, solved, case):
    pb, a = solved[case.name]
    b = ceres_solve(ceres, oracle, pb, oracle.ba_default_options(**case.options))
    print("\n  %-34s Ceres:  %-9s %d iterations, %s, %d successful: %s" % (case.name, TC.pattern(b["trace"]), b["iterations"], NAMES[b["termination"]],
                                                                            b["num_successful_steps"], b["message"]), end="")
    assert (b["iterations"], b["termination"], b["num_successful_steps"], TC.pattern(b["trace"])) == (case.iterations, case.termination, case.successful, case.pattern)
    same_solve(a, b, 1e-9, case.name)
    assert [t["trust_region_radius"] for t in a["trace"]] == [t["trust_region_radius"] for t in b["trace"]]
    if case.kind in ("all_invalid", "unchanged"):
        assert TC.inputs_returned(case, pb, b) and b["final_cost"] == b["initial_cost"]
