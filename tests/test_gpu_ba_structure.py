"""The device BA solvers on problems of IRREGULAR structure (tests/ba_cases.py) against the oracle: landmarks of 0 .. 129 residual
blocks side by side (the lineariser pairs landmarks of at most 32 blocks, reduces a second half-wave above 32 and reads further
batches of 64 straight from memory), shuffled block order (ba_create's sort and res_orig), per-block sigma, calib_r != calib_l, a
rotated T_rl, constant keyframes anywhere, a free keyframe without blocks, left-only / right-only observers, landmarks that lose every
block in localBA's first pass.  The bar is tests/test_gpu_ba.py's, unchanged: 1e-7 on the parameters, identical iteration counts,
terminations, depth flags and outlier sets.  tests/test_ba_cases.py shows on the oracle alone that these problems leave that bar
five orders of margin."""
import numpy as np
import pytest

import ov2slam_amd
from ov2slam_amd import synth, optimizer
from tests import ba_cases as B
from tests.test_gpu_ba import _cmp
from tests.test_gpu_ba_batch import _same
from tests.test_gpu_xyz_ba import _cmp as _cmp_xyz

pytestmark = pytest.mark.gpu

OPTION_SETS = (dict(), dict(max_iter=10, huber_delta=-1.0), dict(max_iter=12, function_tolerance=1e-9))
PATHS = {"default": dict(), "large": dict(ba_force_large=1), "large_direct_chunked": dict(ba_force_large=1, ba_lin_direct=1, ba_schur_chunk=36),
         "deterministic": dict(ba_deterministic=1)}
BITS = ("poses", "invdepth", "chi2", "depthpos")


def _diff(g, r, key="invdepth"):
    """(largest pose difference, largest landmark difference) of a device result against the oracle's"""
    return float(np.abs(g["poses"] - r["poses"]).max()) if "poses" in r else 0.0, float(np.abs(g[key] - r[key]).max())


def _oracle_solver(oracle, xyz=False):
    f = oracle.xyz_ba_solve if xyz else oracle.ba_solve

    def solver(prob, res_active, chi2_init, depthpos_init, **kw):
        return f(prob, oracle.ba_default_options(**kw), res_active, chi2_init, depthpos_init)
    return solver


def _lost(pb, bad, key="res_lm"):
    """landmarks with blocks, all of them bad"""
    n_bad = np.bincount(pb[key][bad], minlength=len(pb["counts"]))
    return np.nonzero((pb["counts"] > 0) & (n_bad == pb["counts"]))[0]


def _by_sorted_order(g, perm):
    """a result on a shuffled problem with its per-block outputs in the order of the problem it was shuffled from"""
    out = dict(g)
    for k in ("chi2", "depthpos", "bad_obs", "bad_after_pass1"):
        if k in g:
            out[k] = B.unshuffle(g[k], perm)
    return out


@pytest.fixture(scope="module")
def irregular(oracle):
    """the standard irregular inverse-depth problem, the oracle's solves under the three option sets, the oracle's localBA"""
    pb = B.irregular_invdepth()
    refs = [oracle.ba_solve(pb, oracle.ba_default_options(**kw)) for kw in OPTION_SETS]
    proto = ov2slam_amd.Optimizer(None, solver=_oracle_solver(oracle)).localBA(pb)
    return pb, refs, proto


@pytest.mark.parametrize("path", list(PATHS))
def test_irregular_problem_matches_oracle(gpu_ctx, irregular, path, capsys):
    pb, refs, _ = irregular
    fixed = np.nonzero(pb["kf_const"])[0].tolist() + [pb["empty_kf"]]
    worst = (0.0, 0.0)
    with gpu_ctx.options(**PATHS[path]):
        for kw, r in zip(OPTION_SETS, refs):
            g = optimizer.solve(gpu_ctx, pb, optimizer.default_options(gpu_ctx.lib, **kw))
            worst = tuple(max(a, b) for a, b in zip(worst, _diff(g, r)))
            with capsys.disabled():
                print("\n  irregular problem, %s path, %s: device - oracle: poses %.2e, inverse depths %.2e" % ((path, kw) + _diff(g, r)), end="")
            _cmp(g, r, pb)
            assert g["final_cost"] < 0.5 * g["initial_cost"]
            # constant keyframes and the free keyframe without blocks: not one bit moves; nor does a landmark without blocks
            assert np.array_equal(g["poses"][fixed], pb["poses"][fixed])
            assert np.array_equal(g["invdepth"][pb["counts"] == 0], pb["invdepth"][pb["counts"] == 0])
            if path == "deterministic":
                g2 = optimizer.solve(gpu_ctx, pb, optimizer.default_options(gpu_ctx.lib, **kw))
                for k in BITS:
                    assert np.array_equal(g2[k], g[k]), k
                assert g2["final_cost"] == g["final_cost"] and g2["initial_cost"] == g["initial_cost"]
    with capsys.disabled():
        print("\n  irregular problem, %s path: largest device - oracle difference: poses %.2e, inverse depths %.2e" % ((path,) + worst))


@pytest.mark.parametrize("c", B.SWEEP_COUNTS)
def test_count_sweep_matches_oracle(gpu_ctx, oracle, c):
    """every landmark with c residual blocks: one count per case, so that a failure names the count"""
    pb = B.count_sweep_problem(c)
    for kw in OPTION_SETS:
        r = oracle.ba_solve(pb, oracle.ba_default_options(**kw))
        for big in (0, 1):
            with gpu_ctx.options(ba_force_large=big):
                _cmp(optimizer.solve(gpu_ctx, pb, optimizer.default_options(gpu_ctx.lib, **kw)), r, pb)


def _large_shuffled(n_lm):
    return B.shuffle_blocks(synth.make_ba_problem(30, n_lm, 21, stereo=True, seed=n_lm), seed=5)


@pytest.mark.parametrize("size", ["irregular", "69700 blocks", "135300 blocks"])
def test_block_order_does_not_matter(gpu_ctx, oracle, irregular, size):
    """The device on a shuffled problem against the device on the same problem sorted by landmark: identical decisions, chi2 and depth
    flags block by block THROUGH the permutation (res_orig), parameters within the bar.  From 65 536 blocks ba_create sorts on 2 host
    threads, from 131 072 on 4, each with its own fill cursors."""
    if size == "irregular":
        pb, ps, sets = irregular[0], B.irregular_invdepth(shuffle=False), OPTION_SETS
    else:
        pb = _large_shuffled(1700 if size.startswith("69700") else 3300)
        ps = {k: (B.unshuffle(v, pb["perm"]) if k.startswith("res_") or k == "is_outlier" else v) for k, v in pb.items()}
        sets = (dict(max_iter=3),)
        assert pb["n_res"] == int(size.split()[0]) and np.all(np.diff(ps["res_lm"]) >= 0) and (np.diff(pb["res_lm"]) < 0).sum() > pb["n_res"] // 4
    for kw in sets:
        g = optimizer.solve(gpu_ctx, pb, optimizer.default_options(gpu_ctx.lib, **kw))
        s = optimizer.solve(gpu_ctx, ps, optimizer.default_options(gpu_ctx.lib, **kw))
        _cmp(_by_sorted_order(g, pb["perm"]), s, ps)
        if size != "irregular":
            _cmp(g, oracle.ba_solve(pb, oracle.ba_default_options(**kw)), pb)
    # both passes of localBA on the resident problem: the outlier verdicts come back through res_orig too
    g, s = ov2slam_amd.Optimizer(gpu_ctx).localBA(pb), ov2slam_amd.Optimizer(gpu_ctx).localBA(ps)
    _same(_by_sorted_order(g, pb["perm"]), s)


@pytest.mark.parametrize("path", ["default", "large", "deterministic"])
def test_irregular_localba_protocol_matches_oracle(gpu_ctx, irregular, path):
    pb, _, r = irregular
    with gpu_ctx.options(**PATHS[path]):
        g = ov2slam_amd.Optimizer(gpu_ctx).localBA(pb)
        g2 = ov2slam_amd.Optimizer(gpu_ctx).localBA_two_calls(pb)
    assert g["l2_done"] and g2["l2_done"] and r["l2_done"]
    for k in ("bad_after_pass1", "bad_obs"):
        assert np.array_equal(g[k], r[k]) and np.array_equal(g2[k], r[k]), k
    _cmp(g2["pass1"], r["pass1"], pb)
    _cmp(g2["pass2"], r["pass2"], pb)
    assert g["iterations"] == (r["pass1"]["iterations"], r["pass2"]["iterations"])
    assert g["termination"] == (r["pass1"]["termination"], r["pass2"]["termination"])
    _cmp(dict(g, iterations=g["iterations"][1], termination=g["termination"][1], final_cost=g["final_cost"][1],
              initial_cost=g["initial_cost"][1], num_successful_steps=g["num_successful_steps"][1]), r["pass2"], pb)
    # the landmarks that lost every block in pass 1: the oracle's, the dead ones among them; pass 2 leaves them where pass 1 put them
    lost = _lost(pb, g["bad_after_pass1"])
    assert np.array_equal(lost, _lost(pb, r["bad_after_pass1"])) and set(pb["dead"]) <= set(lost) and len(lost) >= 3
    assert np.array_equal(g2["pass2"]["invdepth"][lost], g2["pass1"]["invdepth"][lost])
    fixed = np.nonzero(pb["kf_const"])[0].tolist() + [pb["empty_kf"]]
    assert np.array_equal(g["poses"][fixed], pb["poses"][fixed])


def test_batch_of_irregular_and_regular_problems(gpu_ctx, oracle, irregular):
    """ov2_local_ba_batch over irregular problems, regular ones and a tiny one, one irregular problem under a stop request: per problem
    what the single call returns, and for the irregular ones what the oracle's protocol returns"""
    pbs = [irregular[0], synth.make_ba_problem(12, 400, 8, stereo=True, seed=3), B.irregular_invdepth(2), synth.make_ba_problem(6, 40, 4, stereo=False, seed=1),
           synth.make_ba_problem(15, 800, 8, stereo=False, seed=7), B.irregular_invdepth(3)]
    stop = [False, False, False, False, False, True]
    res, nb = ov2slam_amd.Optimizer(gpu_ctx).localBA_batch(pbs, stop=stop)
    assert nb == len(pbs)
    for i, pb in enumerate(pbs):
        one = ov2slam_amd.Optimizer(gpu_ctx)
        ref = ov2slam_amd.Optimizer(None, solver=_oracle_solver(oracle))
        if stop[i]:
            one.signalStopLocalBA(); ref.signalStopLocalBA()
        _same(res[i], one.localBA(pb))
        if "counts" in pb:
            r = ref.localBA(pb)
            assert res[i]["l2_done"] == r["l2_done"] == (not stop[i])
            assert np.array_equal(res[i]["bad_after_pass1"], r["bad_after_pass1"]) and np.array_equal(res[i]["bad_obs"], r["bad_obs"])
            assert res[i]["iterations"] == (r["pass1"]["iterations"], r["pass2"]["iterations"] if r["l2_done"] else 0)
            assert np.abs(res[i]["poses"] - r["poses"]).max() <= 1e-7 * max(1.0, np.abs(r["poses"]).max())
            assert np.allclose(res[i]["invdepth"], r["invdepth"], rtol=1e-6, atol=1e-12)
            lost = _lost(pb, res[i]["bad_after_pass1"])
            assert set(pb["dead"]) <= set(lost) and np.array_equal(lost, _lost(pb, r["bad_after_pass1"]))


def test_irregular_point_problem_matches_oracle(gpu_ctx, oracle):
    """The 3-D point form: points of 1, 2, 63, 64, 65 and 129 blocks among small ones, shuffled; every lineariser width and the HBM
    factorisation.  Option sets: the robust default and the 10-iteration L2 solve; a third, longer robust solve is left out because
    the two dead points -- observed twice with errors nothing can absorb -- keep drifting away under Huber's linear loss (1e5 m after
    12 iterations on the oracle), and what is compared then is how far a point has drifted.  localBA removes their blocks after pass 1."""
    pb = B.irregular_xyz()
    fixed = np.nonzero(pb["kf_const"])[0].tolist() + [pb["empty_kf"]]
    for kw in OPTION_SETS[:2]:
        r = oracle.xyz_ba_solve(pb, oracle.ba_default_options(**kw))
        for opts in (dict(ba_xyz_lin_waves=0), dict(ba_xyz_lin_waves=1), dict(ba_xyz_lin_waves=2), dict(ba_force_large=1)):
            with gpu_ctx.options(**opts):
                g = optimizer.solve_xyz(gpu_ctx, pb, optimizer.default_options(gpu_ctx.lib, **kw))
            _cmp_xyz(g, r)
            assert np.array_equal(g["poses"][fixed], pb["poses"][fixed]) and np.array_equal(g["xyz"][pb["counts"] == 0], pb["xyz"][pb["counts"] == 0])
    g = ov2slam_amd.Optimizer(gpu_ctx).localBA(pb)
    r = ov2slam_amd.Optimizer(None, solver=_oracle_solver(oracle, xyz=True)).localBA(pb)
    assert g["l2_done"] and r["l2_done"]
    assert np.array_equal(g["bad_after_pass1"], r["bad_after_pass1"]) and np.array_equal(g["bad_obs"], r["bad_obs"])
    _cmp_xyz(g["pass1"], r["pass1"]); _cmp_xyz(g["pass2"], r["pass2"])
    lost = _lost(pb, g["bad_after_pass1"], "res_pt")
    assert set(pb["dead"]) <= set(lost) and np.array_equal(g["pass2"]["xyz"][lost], g["pass1"]["xyz"][lost])


def test_irregular_structure_only_problem_matches_oracle(gpu_ctx, oracle):
    pb = B.irregular_structure()
    for kw in (dict(max_iter=10, function_tolerance=1e-3, huber_delta=float(np.sqrt(5.9915))), dict(max_iter=30, function_tolerance=1e-9, huber_delta=-1.0)):
        g = optimizer.structure_only_ba(gpu_ctx, pb, optimizer.default_options(gpu_ctx.lib, **kw))
        r = oracle.structure_ba(pb, oracle.ba_default_options(**kw))
        assert g["iterations"] == r["iterations"] and g["termination"] == r["termination"], (g["iterations"], r["iterations"])
        assert g["num_successful_steps"] == r["num_successful_steps"]
        assert abs(g["initial_cost"] - r["initial_cost"]) <= 1e-10 * abs(r["initial_cost"])
        assert abs(g["final_cost"] - r["final_cost"]) <= 1e-8 * abs(r["final_cost"])
        assert np.abs(g["xyz"] - r["xyz"]).max() <= 1e-7 * max(1.0, np.abs(r["xyz"]).max())
        assert np.allclose(g["chi2"], r["chi2"], rtol=1e-6, atol=1e-9) and np.array_equal(g["depthpos"], r["depthpos"])
        assert np.array_equal(g["xyz"][pb["counts"] == 0], pb["xyz"][pb["counts"] == 0])
