"""Named cases that drive the trust-region loop of every device solver (csrc/ba_core.hpp: d_ctl_iter_begin, d_ctl_candidate,
d_ctl_decide) through the exits and the invalid-step handling that ordinary problems never reach.  Plain data: no GPU, no library.
tests/test_trlm_cases.py runs every case on the oracle (and the `ba` ones on Ceres' own loop), tests/test_gpu_trlm_exits.py on the
device.

All inputs are finite and every decision is deterministic.

DENORMAL RADIUS (initial_radius 1e-310, no radius floor, all tolerances 0).  diag / radius overflows for every column, the
factorisation meets an infinite pivot, every step is invalid: the radius goes 1e-310, 5e-311, 1.25e-311, 1.5625e-312, 9.765625e-314
(halved, quartered, ...: the decrease factor doubles) and the fifth invalid step in a row ends the solve with INVALID_STEPS.  Nothing
moves: outputs are the inputs bit for bit.  Variants: a smaller invalid budget, an iteration budget inside the invalid run
(NO_CONVERGENCE), a radius floor the shrinking radius falls through (MIN_RADIUS).

STEP LOST IN ROUNDING (initial_radius 1e-305).  The solve succeeds, the step is smaller than half an ulp of every parameter, its
norm is exactly 0 and 0 <= parameter_tolerance * (x_norm + parameter_tolerance) = 0 holds although x_norm is still "invalid" (-1):
PARAMETER_TOL on the first step.

RECOVERY (initial_radius ~1e306, max_radius 1e308, min_lm_diagonal 1e-20) on a problem with a free keyframe that no block touches.
That keyframe's pivot is exactly q = fl(min_lm_diagonal / radius): 0 while the quotient rounds to zero (invalid step), a positive
denormal once the invalid steps have shrunk the radius (the step succeeds, num_invalid and the decrease factor are reset, the radius
triples), then 0 again.  Whether q is 0 is decided by one rounding at 2^-1075.  Write u = (min_lm_diagonal / radius) / 2^-1075 for
the exact quotient in units of that boundary: the step is invalid for u < 1.  A case is safe against any other correctly rounded
way of forming q when every u of a radius a linear solve ran at (trace[k] for k < iterations) is below 1/2 or above 2.

  recover_function_tol   initial_radius 6e305:   u = 0.0067, 0.013, 0.054, 0.43 | 6.9, 2.3         all outside (1/2, 2)
  budget3                initial_radius 2.4e306: u = 0.0017, 0.0034, 0.013                         all outside (1/2, 2)
  recover_then_invalid   initial_radius 2.4e306: u = 0.0017, 0.0034, 0.013, 0.11 | 1.73 | 0.58     the last two are inside

The last case is the one with invalid -> success -> invalid, and no initial radius gives it the factor 2: the radius grows by at
most 3 per accepted step (LevenbergMarquardtStrategy::StepAccepted), so the valid step before the boundary and the invalid one after
it have u_a / u_b <= 3 and min(u_a, 1 / u_b) <= sqrt(3) = 1.73.  2.4e306 puts them at 1.727 and 1 / 0.5757 = 1.737, within half a
percent of that optimum; max_iter = 6 ends the solve there, because the halved radius of the next step would sit at u = 1.15.
(1e306, 1e304 and 8 iterations -- patterns SiiiiSSii and SiiSSii -- pass the boundary at u = 0.92 and u = 1.08 and are left out.)
RECOVERY_MARGIN names the margin each case is held to.

TOLERANCE EXITS.  GRADIENT_TOL after three accepted steps and PARAMETER_TOL on the third step, per solver.  Each tolerance is the
geometric middle of the range of tolerances over which the oracle takes that very exit (found by a scan in steps of 10^(1/4)); for
the traced solvers it lies between two consecutive recorded gradient norms, stated beside the case.  TOL_MARGIN is the factor by
which the tolerance may move either way without changing the oracle's decision; tests/test_trlm_cases.py checks it."""
import collections

import numpy as np

from ov2slam_amd import synth
from tests import ba_cases as B

TERM = dict(NO_CONVERGENCE=0, FUNCTION_TOL=1, PARAMETER_TOL=2, GRADIENT_TOL=3, MIN_RADIUS=4, INVALID_STEPS=5)

# solver: "ba" (ov2_ba_solve / oracle.ba_solve, traced; also Ceres' own loop), "xyz" (ov2_xyz_ba_solve), "struct" (ov2_structure_ba)
# kind: "all_invalid" (no step is ever taken: outputs are the inputs, the last evaluated point is the initial one),
#       "unchanged" (a step is evaluated but none is taken: outputs are the inputs), "moves"
# tol: the option whose value decides the exit with a margin of TOL_MARGIN, or None
# margin: for recovery cases the factor every used quotient keeps from the rounding boundary, else None
Case = collections.namedtuple("Case", "name solver problem options pattern iterations termination successful kind tol margin")

PROBLEMS = {
    "ba": lambda: synth.make_ba_problem(8, 200, 6, stereo=True, seed=5),
    "pnp": lambda: synth.make_pnp_problem(120, seed=2),                      # one pose, pose-only blocks: k_ba_pose_only
    "xyz": lambda: synth.make_xyz_ba_problem(5, 30, 4, stereo=True, seed=1),
    "struct": lambda: synth.make_structure_problem(5, 40, 4, seed=1),
    "irregular": B.irregular_invdepth,                                       # 70 keyframes, keyframe 41 free and without blocks
    "recovery_xyz": B.recovery_xyz,                                          # 10 keyframes, keyframe 6 free and without blocks
}

DENORMAL = dict(initial_radius=1e-310, min_radius=0.0, function_tolerance=0.0, parameter_tolerance=0.0, gradient_tolerance=0.0)
LOST = dict(DENORMAL, initial_radius=1e-305)
RECOVERY = dict(max_radius=1e308, min_lm_diagonal=1e-20)
LONG = dict(function_tolerance=1e-12, max_iter=10)
TOL_MARGIN = 1.5
RECOVERY_MARGIN = 2.0
SQRT3_MARGIN = 1.72                                                          # the documented exception: the optimum is sqrt(3)
T = TERM


def _c(name, solver, problem, options, pattern, iterations, termination, successful, kind="moves", tol=None, margin=None):
    return Case(name, solver, problem, options, pattern, iterations, T[termination], successful, kind, tol, margin)


def _invalid_family(tag, solver, problem, traced):
    """the denormal-radius cases and the lost step, the same for every solver"""
    p = (lambda s: s) if traced else (lambda s: None)
    return [
        _c(tag + "/denormal", solver, problem, dict(DENORMAL), p("Siiii"), 5, "INVALID_STEPS", 1, "all_invalid"),
        _c(tag + "/denormal_budget2", solver, problem, dict(DENORMAL, max_consecutive_invalid_steps=2), p("Si"), 2, "INVALID_STEPS", 1, "all_invalid"),
        _c(tag + "/denormal_max_iter3", solver, problem, dict(DENORMAL, max_iter=3), p("Siii"), 3, "NO_CONVERGENCE", 1, "all_invalid"),
        # radius 9.765625e-314 <= 1e-312 after four invalid steps
        _c(tag + "/denormal_min_radius", solver, problem, dict(DENORMAL, min_radius=1e-312), p("Siiii"), 4, "MIN_RADIUS", 1, "all_invalid"),
        _c(tag + "/step_lost", solver, problem, dict(LOST), p("S"), 1, "PARAMETER_TOL", 1, "unchanged"),
    ]


CASES = (
    _invalid_family("ba", "ba", "ba", True)
    + [
        # gradient max norms of the accepted points: 3.623e4, 5834, 1014, 335.1, ...: sqrt(1014 * 335.1) = 582.9
        _c("ba/gradient_tol", "ba", "ba", dict(LONG, gradient_tolerance=582.9), "SSSS", 3, "GRADIENT_TOL", 4, tol="gradient_tolerance"),
        # PARAMETER_TOL on the third step for parameter_tolerance in 1.78e-4 .. 1e-3
        _c("ba/parameter_tol", "ba", "ba", dict(LONG, parameter_tolerance=4.2e-4), "SSS", 3, "PARAMETER_TOL", 3, tol="parameter_tolerance"),
        # relative cost changes of the steps after the recovery: 0.82, 0.033, 2.6e-4: sqrt(0.82 * 0.033) = 0.164
        _c("irregular/recover_function_tol", "ba", "irregular", dict(RECOVERY, initial_radius=6e305, function_tolerance=0.164, max_iter=8),
           "SiiiiS", 6, "FUNCTION_TOL", 2, margin=RECOVERY_MARGIN),
        _c("irregular/recover_then_invalid", "ba", "irregular", dict(RECOVERY, initial_radius=2.4e306, max_iter=6),
           "SiiiiSi", 6, "NO_CONVERGENCE", 2, margin=SQRT3_MARGIN),
        _c("irregular/budget3", "ba", "irregular", dict(RECOVERY, initial_radius=2.4e306, max_consecutive_invalid_steps=3),
           "Sii", 3, "INVALID_STEPS", 1, "all_invalid", margin=RECOVERY_MARGIN),
    ]
    + _invalid_family("pnp", "ba", "pnp", True)
    + [
        # gradient max norms: 811, 1042, 58.12, 3.359, ...: sqrt(58.12 * 3.359) = 13.97
        _c("pnp/gradient_tol", "ba", "pnp", dict(LONG, gradient_tolerance=13.97), "SSSS", 3, "GRADIENT_TOL", 4, tol="gradient_tolerance"),
        # PARAMETER_TOL on the third step for parameter_tolerance in 5.62e-4 .. 3.16e-3
        _c("pnp/parameter_tol", "ba", "pnp", dict(LONG, parameter_tolerance=1.3e-3), "SSS", 3, "PARAMETER_TOL", 3, tol="parameter_tolerance"),
    ]
    + _invalid_family("xyz", "xyz", "xyz", False)
    + [
        # GRADIENT_TOL after three accepted steps for gradient_tolerance in 10 .. 31.6
        _c("xyz/gradient_tol", "xyz", "xyz", dict(LONG, gradient_tolerance=17.8), None, 3, "GRADIENT_TOL", 4, tol="gradient_tolerance"),
        # PARAMETER_TOL on the third step for parameter_tolerance in 1.78e-3 .. 1e-2
        _c("xyz/parameter_tol", "xyz", "xyz", dict(LONG, parameter_tolerance=4.2e-3), None, 3, "PARAMETER_TOL", 3, tol="parameter_tolerance"),
        # no trace: the radii of the invalid run are initial_radius / (1, 2, 8, 64, 1024) by construction, the same u as above
        _c("recovery_xyz/recover", "xyz", "recovery_xyz", dict(RECOVERY, initial_radius=6e305, max_iter=5), None, 5, "NO_CONVERGENCE", 2),
        _c("recovery_xyz/recover_then_invalid", "xyz", "recovery_xyz", dict(RECOVERY, initial_radius=2.4e306, max_iter=6), None, 6, "NO_CONVERGENCE", 2),
        _c("recovery_xyz/budget3", "xyz", "recovery_xyz", dict(RECOVERY, initial_radius=2.4e306, max_consecutive_invalid_steps=3),
           None, 3, "INVALID_STEPS", 1, "all_invalid"),
    ]
    + _invalid_family("struct", "struct", "struct", False)
    + [
        # GRADIENT_TOL after three accepted steps for gradient_tolerance in 1.78 .. 56.2, after four in 0.56 .. 1.4
        _c("struct/gradient_tol", "struct", "struct", dict(LONG, gradient_tolerance=10.0), None, 3, "GRADIENT_TOL", 4, tol="gradient_tolerance"),
        _c("struct/gradient_tol_1", "struct", "struct", dict(LONG, gradient_tolerance=1.0), None, 4, "GRADIENT_TOL", 5),
        # PARAMETER_TOL on the third step for parameter_tolerance in 1.78e-4 .. 3.16e-3
        _c("struct/parameter_tol", "struct", "struct", dict(LONG, parameter_tolerance=1e-3), None, 3, "PARAMETER_TOL", 3, tol="parameter_tolerance"),
        _c("struct/min_radius_at_once", "struct", "struct", dict(min_radius=2e4), None, 0, "MIN_RADIUS", 1, "all_invalid"),
    ]
)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def boundary_units(min_lm_diagonal, radius):
    """u = (min_lm_diagonal / radius) / 2^-1075, exact up to the final conversion (the quotient itself is not a double)"""
    from fractions import Fraction
    return float(Fraction(min_lm_diagonal) / Fraction(radius) * 2 ** 1075)


def pattern(trace):
    return "".join("S" if t["step_is_successful"] else ("r" if t["step_is_valid"] else "i") for t in trace)


def landmark_key(case):
    return "invdepth" if case.solver == "ba" else "xyz"


def oracle_solve(oracle, case, problem, **override):
    """the case on the oracle (ba: with the trace)"""
    opts = oracle.ba_default_options(**dict(case.options, **override))
    if case.solver == "ba":
        return oracle.ba_solve(problem, opts, trace=True)
    return (oracle.xyz_ba_solve if case.solver == "xyz" else oracle.structure_ba)(problem, opts)


def inputs_returned(case, problem, result):
    """outputs equal the inputs bit for bit"""
    same = np.array_equal(np.asarray(result[landmark_key(case)]).reshape(-1), np.asarray(problem[landmark_key(case)], np.float64).reshape(-1))
    if case.solver != "struct":
        same = same and np.array_equal(result["poses"], np.asarray(problem["poses"], np.float64).reshape(-1, 7))
    return bool(same)
