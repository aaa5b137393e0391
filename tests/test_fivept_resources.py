"""k_e5_solve / k_e5_score / k_e5_pick (ov2slam_amd/csrc/fivept.hip): a device-only compile for gfx950 shows no scratch in any of
the three (the register counts are printed and recorded in DESIGN.md 4.11, not bounded), and the C ABI of the relative-pose search
rejects bad arguments without a GPU and without writing its outputs (the inputs are checked before the context)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import fivept_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
TH = R.threshold_of(3.0, 460.0, 460.0)
OUTPUTS = ("outliers", "trace_valid", "trace_score", "trace_model")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_fivept_kernels_use_no_scratch(tmp_path):
    src = os.path.join(ROOT, "ov2slam_amd", "csrc", "fivept.hip")
    out = str(tmp_path / "fivept.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                    "--cuda-device-only", "-S", src, "-o", out], check=True, capture_output=True)
    txt = open(out).read()
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        res[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)\s", m.group(2))}
    names = sorted(n for n in res if "k_e5_" in n)
    assert len(names) == 3 and all(any(k in n for n in names) for k in ("k_e5_solve", "k_e5_score", "k_e5_pick")), names
    for n in names:
        print(n, "vgpr", res[n]["next_free_vgpr"], "sgpr", res[n]["next_free_sgpr"], "lds", res[n]["group_segment_fixed_size"])
        assert res[n]["private_segment_fixed_size"] == 0, (n, res[n])
        assert res[n]["group_segment_fixed_size"] <= 65536


def _lib():
    import ov2slam_amd
    return ov2slam_amd.load()


def _call(problem=None, batch=False, n_items=1, null=(), **params):
    """the call with a NULL context on a well-formed 16-point problem, modified: (return code, message)"""
    from ov2slam_amd import pose
    rng = np.random.default_rng(5)
    bv1, bv2, _, _, _ = R.make_scene(rng, 16)
    pb = dict(bv1=bv1, bv2=bv2, samples=R.draw_samples(1, 16, 10))
    pb.update(problem or {})
    args = dict(max_iterations=10, threshold=TH)
    args.update(params)
    s, r, keep = pose._epi_problem(pb, True)
    for a in OUTPUTS:
        keep[a].view(np.uint8)[...] = 0xEE
    for f in null:
        setattr(s if hasattr(s, f) else r, f, None)
    lib = _lib()
    P = pose.epipolar_params(**args)
    if batch:
        rc = lib.ov2_epipolar_ransac_batch(None, C.byref(P), n_items, C.byref(s), C.byref(r))
    else:
        rc = lib.ov2_epipolar_ransac(None, C.byref(P), C.byref(s), C.byref(r))
    assert all((keep[a].view(np.uint8) == 0xEE).all() for a in OUTPUTS), "a rejected call wrote its outputs"
    return rc, lib.ov2_last_error()


def test_null_arguments_are_einval():
    from ov2slam_amd import _lib as L
    lib = _lib()
    p, s, r = L.EpipolarParams(), L.EpipolarProblem(), L.EpipolarResult()
    assert lib.ov2_epipolar_ransac(None, None, None, None) == L.OV2_EINVAL and b"NULL" in lib.ov2_last_error()
    assert lib.ov2_epipolar_ransac(None, C.byref(p), None, C.byref(r)) == L.OV2_EINVAL
    assert lib.ov2_epipolar_ransac(None, C.byref(p), C.byref(s), None) == L.OV2_EINVAL
    assert lib.ov2_epipolar_ransac_batch(None, None, 1, C.byref(s), C.byref(r)) == L.OV2_EINVAL and b"NULL params" in lib.ov2_last_error()
    rc, msg = _call(batch=True, n_items=-1)
    assert rc == L.OV2_EINVAL and b"n_items" in msg
    rc, msg = _call(batch=True, n_items=65536)
    assert rc == L.OV2_EINVAL and b"65535" in msg
    assert lib.ov2_epipolar_draw_samples(1, 9, 2, None) == L.OV2_EINVAL
    assert lib.ov2_epipolar_draw_samples(1, 7, 2, (C.c_int * 16)()) == L.OV2_EINVAL
    assert lib.ov2_epipolar_draw_samples(1, 9, -1, (C.c_int * 16)()) == L.OV2_EINVAL


def test_well_formed_input_reaches_the_context_check():
    from ov2slam_amd import _lib as L
    for batch in (False, True):
        rc, msg = _call(batch=batch)
        assert rc == L.OV2_EINVAL and b"NULL context" in msg, msg
    # fewer than eight points, no points, no rows, rows of bad indices: not errors
    z7 = np.zeros((7, 3)) + [0, 0, 1.0]
    for pb in (dict(bv1=z7, bv2=z7, samples=np.zeros((0, 8), np.int32)),
               dict(bv1=np.zeros((0, 3)), bv2=np.zeros((0, 3)), samples=np.zeros((0, 8), np.int32)),
               dict(samples=np.zeros((0, 8), np.int32)), dict(samples=np.array([[0, 0, 99, -1, 1, 2, 3, 4]], np.int32))):
        rc, msg = _call(problem=pb)
        assert rc == L.OV2_EINVAL and b"NULL context" in msg, msg


BAD = [
    ("threshold_zero", dict(threshold=0.0), {}, (), b"threshold"),
    ("threshold_negative", dict(threshold=-1e-5), {}, (), b"threshold"),
    ("threshold_nan", dict(threshold=float("nan")), {}, (), b"threshold"),
    ("threshold_inf", dict(threshold=float("inf")), {}, (), b"threshold"),
    ("boptimize", dict(boptimize=True), {}, (), b"boptimize"),
    ("max_iterations_negative", dict(max_iterations=-1), {}, (), b"max_iterations"),
    ("probability_one", dict(probability=1.0), {}, (), b"probability"),
    ("probability_zero", dict(probability=0.0), {}, (), b"probability"),
    ("bv1_nan", {}, "bv1_nan", (), b"not finite"),
    ("bv2_inf", {}, "bv2_inf", (), b"not finite"),
    ("too_many_points", {}, "points", (), b"capacity"),
    ("too_many_rows", {}, "rows", (), b"capacity"),
    ("null_bv1", {}, {}, ("bv1",), b"NULL bv1"),
    ("null_bv2", {}, {}, ("bv2",), b"NULL bv1 / bv2"),
    ("null_samples", {}, {}, ("samples",), b"NULL samples"),
    ("null_outliers", {}, {}, ("outliers",), b"result buffer"),
]


def _problem_of(kind):
    if not isinstance(kind, str):
        return kind
    rng = np.random.default_rng(5)
    bv1, bv2, _, _, _ = R.make_scene(rng, 16)
    if kind == "bv1_nan":
        bv1[7, 2] = np.nan
        return dict(bv1=bv1)
    if kind == "bv2_inf":
        bv2[15, 0] = -np.inf
        return dict(bv2=bv2)
    if kind == "points":
        z = np.tile([0, 0, 1.0], (R.MAX_POINTS + 1, 1))
        return dict(bv1=z, bv2=z)
    return dict(samples=np.zeros((R.MAX_ROWS + 1, 8), np.int32))


@pytest.mark.parametrize("batch", [False, True], ids=["single", "batch"])
@pytest.mark.parametrize("case", BAD, ids=lambda c: c[0])
def test_invalid_input_is_rejected_without_a_gpu(case, batch):
    from ov2slam_amd import _lib as L
    name, params, problem, null, word = case
    rc, msg = _call(problem=_problem_of(problem), batch=batch, null=null, **params)
    assert rc == L.OV2_EINVAL and word in msg and b"NULL context" not in msg, (name, rc, msg)


def test_negative_counts():
    from ov2slam_amd import _lib as L
    from ov2slam_amd import pose
    lib = _lib()
    rng = np.random.default_rng(5)
    bv1, bv2, _, _, _ = R.make_scene(rng, 16)
    for field in ("n", "n_rows"):
        s, r, keep = pose._epi_problem(dict(bv1=bv1, bv2=bv2, samples=R.draw_samples(1, 16, 10)), False)
        setattr(s, field, -1)
        assert lib.ov2_epipolar_ransac(None, C.byref(pose.epipolar_params(10, TH)), C.byref(s), C.byref(r)) == L.OV2_EINVAL
        assert b"negative count" in lib.ov2_last_error()


def test_capacity_constants_match_the_header():
    from ov2slam_amd import _lib as L
    from ov2slam_amd import pose
    assert L.OV2_EPI_MAX_POINTS == R.MAX_POINTS == pose.EPI_MAX_POINTS == 2048
    assert L.OV2_EPI_MAX_ROWS == R.MAX_ROWS == pose.EPI_MAX_ROWS == 4096
    assert (L.OV2_EPI_TOO_FEW_POINTS, L.OV2_EPI_NO_MODEL, L.OV2_EPI_FEW_INLIERS) == (R.TOO_FEW_POINTS, R.NO_MODEL, R.FEW_INLIERS)
    hdr = open(os.path.join(ROOT, "include", "ov2slam_hip.h")).read()
    assert "#define OV2_EPI_MAX_POINTS %d" % L.OV2_EPI_MAX_POINTS in hdr and "#define OV2_EPI_MAX_ROWS %d" % L.OV2_EPI_MAX_ROWS in hdr
    assert "OV2_EPI_TOO_FEW_POINTS = 1, OV2_EPI_NO_MODEL = 2, OV2_EPI_FEW_INLIERS = 4" in hdr
    z = np.tile([0, 0, 1.0], (R.MAX_POINTS, 1))
    rc, msg = _call(problem=dict(bv1=z, bv2=z, samples=np.zeros((R.MAX_ROWS, 8), np.int32)))
    assert rc == L.OV2_EINVAL and b"NULL context" in msg          # the capacity itself passes every input check
