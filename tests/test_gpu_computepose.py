"""GPU tests of scope row f15 (csrc/pnp.hip): ov2_ceres_pnp[_batch] against ceresPnP's protocol on the oracle, ov2_compute_pose[_batch]
against tests/computepose_ref.py on every named scene, the bit-exact properties (repeats, batch = singles, chain = its parts), the
C++ adapters and the argument checks with a live context.

Bars: the pose within 1e-7 (the project's BA bar, compared as tests/test_gpu_ba.py does); success flags, outlier lists, iteration
counts, successful steps, terminations, actions, flags, removal bytes, counts and P3P's integer scalars identical.  P3P's score is a
float the device and numpy form by different roads: it is held to the bar tests/test_gpu_p3p.py holds it to (TOL_BEST)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ov2slam_amd
from ov2slam_amd import pose
from tests import computepose_ref as R

pytestmark = pytest.mark.gpu

TIGHT = 1e-7
P3P_SCORE_TOL = 2.22e-10          # tests/test_gpu_p3p.py, TOL_BEST
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pose_close(g, r):
    dt = np.abs(g[:3] - r[:3]).max()
    dq = np.abs(g[3:] * np.sign(g[3:] @ r[3:]) - r[3:]).max()
    print("pose: translation %.3g (allowed %.3g), quaternion %.3g (allowed %.3g)" % (dt, TIGHT * max(1.0, np.abs(r[:3]).max()), dq, TIGHT))
    assert dt <= TIGHT * max(1.0, np.abs(r[:3]).max())
    assert dq <= TIGHT


def _passes_equal(g, r):
    for q in range(2):
        for k in ("ran", "iterations", "num_successful_steps", "termination"):
            assert g[q][k] == r[q][k], (q, k, g[q], r[q])
        if r[q]["ran"]:
            assert abs(g[q]["initial_cost"] - r[q]["initial_cost"]) <= 1e-9 * abs(r[q]["initial_cost"]) + 1e-12
            assert abs(g[q]["final_cost"] - r[q]["final_cost"]) <= 1e-7 * abs(r[q]["final_cost"]) + 1e-12


def _bits(res):
    """everything a result holds, as bytes"""
    parts = []
    for k in sorted(res):
        v = res[k]
        if isinstance(v, dict):
            parts.append(_bits(v))
        elif isinstance(v, list):
            parts.extend(_bits(q) for q in v)
        else:
            parts.append(np.ascontiguousarray(v).tobytes())
    return b"".join(parts)


@pytest.mark.parametrize("n", [4, 5, 63, 64, 65, 257, 308])
def test_ceres_pnp_matches_the_reference_protocol(gpu_ctx, oracle, n):
    """the wavefront edge and more points than threads; with and without outliers, robust on and off, apply_l2 on and off"""
    mvg = ov2slam_amd.MultiViewGeometry(gpu_ctx)
    for with_outliers in (False, True):
        for use_robust in (True, False):
            for apply_l2 in (True, False):
                pb, ref = R.pnp_case(oracle, n, with_outliers, use_robust, apply_l2)
                g = pose.ceres_pnp(gpu_ctx, dict(nmaxiter=5, chi2th=R.CHI2TH, use_robust=use_robust, apply_l2_after_robust=apply_l2, K=R.K), pb)
                assert g["success"] == ref["success"]
                assert np.array_equal(g["outliers"], ref["outliers"])
                _passes_equal(g["passes"], ref["passes"])
                _pose_close(g["Twc"], ref["Twc"])
                # the existing two-call route gives the same decisions
                ok2, T2, out2 = mvg.ceresPnP(pb["unpx"], pb["wpt"], pb["scale"], pb["Twc"], 5, R.CHI2TH, use_robust, apply_l2, *[float(v) for v in R.K])
                assert ok2 == g["success"] and np.array_equal(out2, g["outliers"])
                _pose_close(np.asarray(T2, np.float64), ref["Twc"])


def _check_scene(g, ref):
    assert g["action"] == ref["action"], (pose.ACTION_NAMES[g["action"]], pose.ACTION_NAMES[ref["action"]])
    assert g["p3p_req_out"] == ref["p3p_req_out"]
    assert np.array_equal(g["removed"], ref["removed"])
    assert g["n_removed_p3p"] == ref["n_removed_p3p"] and g["n_outliers_pnp"] == ref["n_outliers_pnp"]
    assert g["ran_p3p"] == ref["ran_p3p"]
    for k in ("status", "best_row", "iterations", "rows_consumed"):
        assert g["p3p"][k] == ref["p3p"][k], k
    assert abs(g["p3p"]["score"] - ref["p3p"]["score"]) <= P3P_SCORE_TOL
    _passes_equal(g["passes"], ref["passes"])
    _pose_close(g["Twc"], ref["Twc"])


@pytest.mark.parametrize("name", list(R.SCENES))
def test_compute_pose_on_every_named_scene(gpu_ctx, oracle, name):
    params, pb, ref = R.named_scene(oracle, name)
    g = pose.compute_pose(gpu_ctx, params, pb)
    _check_scene(g, ref)
    if ref["action"] in (R.TOO_FEW, R.P3P_RESET, R.PNP_REQ_P3P):
        assert np.array_equal(g["Twc"].view(np.uint64), np.asarray(pb["Twc"], np.float64).view(np.uint64))     # the pose is untouched


def _eleven(oracle):
    """11 items of different sizes: n = 0, n = 3, one P3P_RESET, one PNP_REQ_P3P, mixed do_p3p.  One params for all (a batch shares
    them), so the items are generated here and not taken from the named scenes with their own params."""
    sk = R.SCENES
    items = [R.make_scene(1, 0), R.make_scene(2, 3, do_p3p=True), R.named_scene(oracle, "p3p_reset_few")[1],
             R.named_scene(oracle, "req_p3p")[1], R.named_scene(oracle, "ok_p3p")[1], R.named_scene(oracle, "ok_no_p3p")[1],
             R.make_scene(3, 65, outlier_frac=0.1, do_p3p=True), R.make_scene(4, 308, outlier_frac=0.05),
             R.make_scene(5, 257, outlier_frac=0.2, do_p3p=True, p3p_req=True), R.named_scene(oracle, "all_behind")[1],
             R.make_scene(6, 600, outlier_frac=0.1, do_p3p=True)]
    assert sk["req_p3p"][1] == {} and sk["ok_p3p"][1] == {} and sk["p3p_reset_few"][1] == {}      # they were made for the default params
    return R.params_of(), items


def test_three_repeats_give_the_same_bits(gpu_ctx, oracle):
    params, items = _eleven(oracle)
    for pb in (items[4], items[7], items[10]):
        a = [_bits(pose.compute_pose(gpu_ctx, params, pb)) for _ in range(3)]
        assert a[0] == a[1] == a[2]
        b = [_bits(pose.ceres_pnp(gpu_ctx, params["pnp"], pb)) for _ in range(3)]
        assert b[0] == b[1] == b[2]


def test_a_batch_of_eleven_equals_eleven_single_calls(gpu_ctx, oracle):
    params, items = _eleven(oracle)
    batch = pose.compute_pose_batch(gpu_ctx, params, items)
    singles = [pose.compute_pose(gpu_ctx, params, pb) for pb in items]
    acts = [s["action"] for s in singles]
    print("actions:", [pose.ACTION_NAMES[a] for a in acts])
    assert acts[0] == acts[1] == R.TOO_FEW and acts[2] == R.P3P_RESET and acts[3] == R.PNP_REQ_P3P and acts.count(R.POSE_OK) >= 4
    for b, (x, y) in enumerate(zip(batch, singles)):
        assert _bits(x) == _bits(y), b
    pb_batch = pose.ceres_pnp_batch(gpu_ctx, params["pnp"], items)
    for b, pb in enumerate(items):
        assert _bits(pb_batch[b]) == _bits(pose.ceres_pnp(gpu_ctx, params["pnp"], pb)), b


def test_seventy_copies_give_seventy_equal_results(gpu_ctx, oracle):
    params, items = _eleven(oracle)
    for pb in (items[4], items[7]):
        got = [_bits(r) for r in pose.compute_pose_batch(gpu_ctx, params, [pb] * 70)]
        assert all(g == got[0] for g in got)
        assert got[0] == _bits(pose.compute_pose(gpu_ctx, params, pb))
        got = [_bits(r) for r in pose.ceres_pnp_batch(gpu_ctx, params["pnp"], [pb] * 70)]
        assert all(g == got[0] for g in got)


def test_the_chain_equals_p3p_then_pnp_on_host_compacted_arrays(gpu_ctx, oracle):
    params, items = _eleven(oracle)
    ran = 0
    for pb in items:
        if not pb["do_p3p"] or len(pb["unpx"]) < 4:
            continue
        g = pose.compute_pose(gpu_ctx, params, pb)
        s = pose.p3p_ransac(gpu_ctx, params["p3p"], dict(bv=pb["bv"], X=pb["wpt"], samples=pb["samples"]))
        assert (g["p3p"]["status"], g["p3p"]["best_row"], g["p3p"]["iterations"], g["p3p"]["rows_consumed"]) == \
               (s["status"], s["best_row"], s["iterations"], s["rows_consumed"])
        assert np.float64(g["p3p"]["score"]).tobytes() == np.float64(s["score"]).tobytes()
        if g["action"] == R.P3P_RESET:
            assert s["status"] != 0 or s["n_inliers"] < 5
            continue
        keep = np.ones(len(pb["unpx"]), bool)
        keep[s["outliers"]] = False
        assert np.array_equal(g["removed"] == 1, ~keep)
        T0 = pose.pose_from_model(s["model"])
        r = pose.ceres_pnp(gpu_ctx, params["pnp"], dict(unpx=pb["unpx"][keep], wpt=pb["wpt"][keep], scale=pb["scale"][keep], Twc=T0))
        assert _bits(dict(p=g["passes"])) == _bits(dict(p=r["passes"]))
        assert g["n_outliers_pnp"] == len(r["outliers"])
        if g["action"] == R.POSE_OK:
            assert g["Twc"].tobytes() == r["Twc"].tobytes()
            assert np.array_equal(np.nonzero(g["removed"] == 2)[0], np.nonzero(keep)[0][r["outliers"]])
        else:
            assert g["Twc"].tobytes() == T0.tobytes()
        ran += 1
    assert ran >= 4


def test_a_rejected_call_with_a_live_context_leaves_the_outputs_untouched(gpu_ctx, oracle):
    from ov2slam_amd import _lib as L
    params, items = _eleven(oracle)
    pb = items[4]
    for entry in ("pnp", "pose"):
        p = pose._as_pnp_params(params["pnp"]) if entry == "pnp" else pose._as_pose_params(params)
        bad = dict(pb, wpt=np.where(np.arange(len(pb["wpt"]))[:, None] == 7, np.nan, pb["wpt"]))
        for case in ("nan", "chi2th"):
            s, r, keep = (pose._pnp_problem if entry == "pnp" else pose._pose_problem)(bad if case == "nan" else pb)
            out = keep["outliers" if entry == "pnp" else "removed"]
            C.memset(C.byref(r), 0x6E, C.sizeof(r))
            if entry == "pnp":
                r.outliers = out.ctypes.data_as(C.POINTER(C.c_int))
            else:
                r.removed = out.ctypes.data_as(C.POINTER(C.c_uint8))
            out.view(np.uint8)[...] = 0x6E
            before = bytes(C.string_at(C.byref(r), C.sizeof(r)))
            q = type(p).from_buffer_copy(p)
            if case == "chi2th":
                (q if entry == "pnp" else q.pnp).chi2th = -1.0
            fn = gpu_ctx.lib.ov2_ceres_pnp if entry == "pnp" else gpu_ctx.lib.ov2_compute_pose
            rc = fn(gpu_ctx.h, C.byref(q), C.byref(s), C.byref(r))
            assert rc == L.OV2_EINVAL
            assert (out.view(np.uint8) == 0x6E).all() and bytes(C.string_at(C.byref(r), C.sizeof(r))) == before
    # and the context still works
    g = pose.compute_pose(gpu_ctx, params, pb)
    assert g["action"] == R.POSE_OK


def _wr(f, a):
    b = np.ascontiguousarray(a).tobytes()
    f.write(np.int64(len(b)).tobytes() + b)


def _rd(f, dtype):
    nb = int(np.frombuffer(f.read(8), np.int64)[0])
    return np.frombuffer(f.read(nb), dtype)


def test_cpp_adapters_give_what_the_python_form_gives(gpu_ctx, oracle, tmp_path):
    """tests/cpp/pose_adapters.cpp: ov2::computePose (single and a batch of two) and ov2::ceresPnPFused return, bit for bit, what
    pose.compute_pose / pose.ceres_pnp return on the same arrays, sample table and (float) camera"""
    exe = tmp_path / "pose_adapters"
    libdir = os.path.join(ROOT, "ov2slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "pose_adapters.cpp"),
                           "-o", str(exe), "-L", libdir, "-lov2slam_hip", "-Wl,-rpath," + libdir])
    pb = R.make_scene(21, 150, outlier_frac=0.1, do_p3p=True, p3p_req=True)
    n, iters, seed, errth = 150, 20, 77, 3.0
    Kf = np.asarray(R.K, np.float32)
    case, res = tmp_path / "case.bin", tmp_path / "res.bin"
    with open(case, "wb") as f:
        _wr(f, np.array([iters, seed, 1, 1, 0, 1], np.int32))
        _wr(f, np.concatenate([[np.float32(errth), np.float32(R.CHI2TH)], Kf]).astype(np.float32))
        for k, t in (("unpx", np.float64), ("wpt", np.float64), ("bv", np.float64), ("Twc", np.float64), ("scale", np.int32)):
            _wr(f, np.asarray(pb[k], t))
    r = subprocess.run([str(exe), str(case), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    params = dict(pnp=dict(nmaxiter=5, chi2th=float(np.float32(R.CHI2TH)), use_robust=True, apply_l2_after_robust=True, K=Kf.astype(np.float64)),
                  p3p=dict(mode=pose.LMEDS, max_iterations=iters, threshold=pose.threshold(errth, Kf[0], Kf[1])), mono=False)
    want = pose.compute_pose(gpu_ctx, params, dict(pb, samples=pose.draw_samples(seed, n, 2 * iters)))
    assert want["action"] == R.POSE_OK and want["n_removed_p3p"] > 0
    wpnp = pose.ceres_pnp(gpu_ctx, params["pnp"], pb)
    with open(res, "rb") as f:
        for _ in range(3):                                           # the single call, then the two items of the batch
            head, T, removed = _rd(f, np.int32), _rd(f, np.float64), _rd(f, np.uint8)
            assert list(head) == [0, want["action"], int(want["p3p_req_out"]), want["n_removed_p3p"], want["n_outliers_pnp"],
                                  want["p3p"]["status"], want["p3p"]["best_row"]]
            assert T.tobytes() == want["Twc"].tobytes() and np.array_equal(removed, want["removed"])
        ok, T, out = _rd(f, np.int32), _rd(f, np.float64), _rd(f, np.int32)
        assert bool(ok[0]) == wpnp["success"] and T.tobytes() == wpnp["Twc"].tobytes() and np.array_equal(out, wpnp["outliers"])
