"""k_pg_solve / k_pg_apply (ov2slam_amd/csrc/posegraph.hip): a device-only compile for gfx950 shows no scratch in either (the
register counts are printed and recorded in DESIGN.md 4.12, not bounded), and the C ABI of the pose-graph solver rejects bad
arguments without a GPU and without writing its outputs (the inputs are checked before the context)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import posegraph_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_posegraph_kernels_use_no_scratch(tmp_path):
    src = os.path.join(ROOT, "ov2slam_amd", "csrc", "posegraph.hip")
    out = str(tmp_path / "posegraph.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                    "--cuda-device-only", "-S", src, "-o", out], check=True, capture_output=True)
    txt = open(out).read()
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        res[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)\s", m.group(2))}
    names = sorted(n for n in res if "k_pg_" in n)
    assert len(names) == 2 and all(any(k in n for n in names) for k in ("k_pg_solve", "k_pg_apply")), names
    for n in names:
        print(n, "vgpr", res[n]["next_free_vgpr"], "sgpr", res[n]["next_free_sgpr"], "lds", res[n]["group_segment_fixed_size"])
        assert res[n]["private_segment_fixed_size"] == 0, (n, res[n])
        assert res[n]["group_segment_fixed_size"] <= 65536


def _lib():
    import ov2slam_amd
    return ov2slam_amd.load()


def _good():
    return R.make_local_scene(np.random.default_rng(3), 6)


def _call(prob=None, batch=False, n_items=1, null=(), set_fields=None, **opt):
    """the call with a NULL context on a well-formed 6-pose problem, modified: (return code, message)"""
    from ov2slam_amd import optimizer as O
    p = _good()
    p.update(prob or {})
    P, Rs, out, keep = O._pg_pack(p)
    out.view(np.uint8)[...] = 0xEE
    before = (Rs.iterations, Rs.termination, Rs.final_cost)
    for f in null:
        setattr(P if hasattr(P, f) else Rs, f, None)
    for f, v in (set_fields or {}).items():
        setattr(P, f, v)
    lib = _lib()
    opts = O.pose_graph_options(lib, **opt)
    if batch:
        rc = lib.ov2_pose_graph_solve_batch(None, n_items, C.byref(P), C.byref(opts), C.byref(Rs))
    else:
        rc = lib.ov2_pose_graph_solve(None, C.byref(P), C.byref(opts), C.byref(Rs))
    assert (out.view(np.uint8) == 0xEE).all() and (Rs.iterations, Rs.termination, Rs.final_cost) == before, "a rejected call wrote its outputs"
    return rc, lib.ov2_last_error()


def test_null_arguments_are_einval():
    from ov2slam_amd import _lib as L
    from ov2slam_amd import optimizer as O
    lib = _lib()
    p, r, o = L.PGProblem(), L.PGResult(), O.pose_graph_options(lib)
    assert lib.ov2_pose_graph_solve(None, None, None, None) == L.OV2_EINVAL and b"NULL" in lib.ov2_last_error()
    assert lib.ov2_pose_graph_solve(None, None, C.byref(o), C.byref(r)) == L.OV2_EINVAL
    assert lib.ov2_pose_graph_solve(None, C.byref(p), C.byref(o), None) == L.OV2_EINVAL
    assert lib.ov2_pose_graph_solve(None, C.byref(p), None, C.byref(r)) == L.OV2_EINVAL and b"NULL options" in lib.ov2_last_error()
    assert lib.ov2_pose_graph_solve_batch(None, 1, None, C.byref(o), C.byref(r)) == L.OV2_EINVAL and b"NULL problem" in lib.ov2_last_error()
    rc, msg = _call(batch=True, n_items=-1)
    assert rc == L.OV2_EINVAL and b"n_items" in msg
    rc, msg = _call(batch=True, n_items=65536)
    assert rc == L.OV2_EINVAL and b"65535" in msg


def _bad_problem(kind):
    p = _good()
    if kind == "pose_nan":
        p["poses"][3, 1] = np.nan
    elif kind == "pose_inf":
        p["poses"][5, 6] = np.inf
    elif kind == "zero_quaternion":
        p["poses"][2, 3:] = 0.0
    elif kind == "measurement_nan":
        p["edge_T"][1, 0] = np.nan
    elif kind == "measurement_zero_quaternion":
        p["edge_T"][4, 3:] = 0.0
    elif kind == "index_high":
        p["edge_j"][2] = 6
    elif kind == "index_negative":
        p["edge_i"][0] = -1
    elif kind == "i_equals_j":
        p["edge_j"][3] = p["edge_i"][3]
    elif kind == "not_neighbours":
        p["edge_i"][2], p["edge_j"][2] = 1, 3                       # both variable, one variable pose between them
    elif kind == "sigma_zero":
        p["edge_sigma"] = np.ones(6); p["edge_sigma"][1] = 0.0
    elif kind == "sigma_inf":
        p["edge_sigma"] = np.ones(6); p["edge_sigma"][5] = np.inf
    elif kind == "too_many_poses":
        n = R.MAX_POSES + 1
        p = dict(poses=np.tile([0, 0, 0, 0, 0, 0, 1.0], (n, 1)), pose_const=np.ones(n, np.uint8), edge_i=np.zeros(1, np.int32),
                 edge_j=np.ones(1, np.int32), edge_T=np.array([[0, 0, 0, 0, 0, 0, 1.0]]))
    elif kind == "too_many_edges":
        m = R.MAX_EDGES + 1
        p = dict(p, edge_i=np.zeros(m, np.int32), edge_j=np.ones(m, np.int32), edge_T=np.tile([0, 0, 0, 0, 0, 0, 1.0], (m, 1)))
    return p


BAD = [
    ("pose_nan", "pose_nan", {}, (), {}, b"not finite", "EINVAL"),
    ("pose_inf", "pose_inf", {}, (), {}, b"not finite", "EINVAL"),
    ("zero_quaternion", "zero_quaternion", {}, (), {}, b"zero quaternion", "EINVAL"),
    ("measurement_nan", "measurement_nan", {}, (), {}, b"measurement not finite", "EINVAL"),
    ("measurement_zero_quaternion", "measurement_zero_quaternion", {}, (), {}, b"zero quaternion", "EINVAL"),
    ("index_high", "index_high", {}, (), {}, b"out of range", "EINVAL"),
    ("index_negative", "index_negative", {}, (), {}, b"out of range", "EINVAL"),
    ("i_equals_j", "i_equals_j", {}, (), {}, b"i == j", "EINVAL"),
    ("not_neighbours", "not_neighbours", {}, (), {}, b"edge 2 (1, 3)", "EUNSUPPORTED"),
    ("sigma_zero", "sigma_zero", {}, (), {}, b"edge_sigma", "EINVAL"),
    ("sigma_inf", "sigma_inf", {}, (), {}, b"edge_sigma", "EINVAL"),
    ("too_many_poses", "too_many_poses", {}, (), {}, b"capacity", "EINVAL"),
    ("too_many_edges", "too_many_edges", {}, (), {}, b"capacity", "EINVAL"),
    ("negative_poses", None, {}, (), dict(n_poses=-1), b"negative count", "EINVAL"),
    ("negative_edges", None, {}, (), dict(n_edges=-1), b"negative count", "EINVAL"),
    ("null_poses", None, {}, ("poses",), {}, b"NULL poses", "EINVAL"),
    ("null_pose_const", None, {}, ("pose_const",), {}, b"NULL poses / pose_const", "EINVAL"),
    ("null_edge_i", None, {}, ("edge_i",), {}, b"NULL edge_i", "EINVAL"),
    ("null_edge_T", None, {}, ("edge_T",), {}, b"NULL edge_i / edge_j / edge_T", "EINVAL"),
    ("null_poses_out", None, {}, ("poses_out",), {}, b"result buffer", "EINVAL"),
    ("huber", None, dict(huber_delta=1.0), (), {}, b"huber_delta", "EUNSUPPORTED"),
    ("solver_time", None, dict(max_solver_time_s=0.01), (), {}, b"max_solver_time_s", "EUNSUPPORTED"),
    ("max_iter_negative", None, dict(max_iter=-1), (), {}, b"max_iter", "EINVAL"),
]


@pytest.mark.parametrize("batch", [False, True], ids=["single", "batch"])
@pytest.mark.parametrize("case", BAD, ids=lambda c: c[0])
def test_invalid_input_is_rejected_without_a_gpu(case, batch):
    from ov2slam_amd import _lib as L
    name, kind, opt, null, fields, word, code = case
    rc, msg = _call(prob=_bad_problem(kind) if kind else None, batch=batch, null=null, set_fields=fields, **opt)
    assert rc == getattr(L, "OV2_" + code) and word in msg and b"NULL context" not in msg, (name, rc, msg)


def test_well_formed_input_reaches_the_context_check():
    from ov2slam_amd import _lib as L
    p = _good()
    allc = dict(pose_const=np.ones(6, np.uint8))
    noedge = dict(edge_i=np.zeros(0, np.int32), edge_j=np.zeros(0, np.int32), edge_T=np.zeros((0, 7)))
    rev = R.reverse_edges(p)
    repeated = dict(edge_i=np.concatenate([p["edge_i"], p["edge_i"][:2]]), edge_j=np.concatenate([p["edge_j"], p["edge_j"][:2]]),
                    edge_T=np.concatenate([p["edge_T"], p["edge_T"][:2]]))
    # variable 1 and variable 3 ARE neighbours among the variable poses once pose 2 is constant
    skip = dict(pose_const=np.array([1, 0, 1, 0, 0, 0], np.uint8), edge_i=np.array([1], np.int32), edge_j=np.array([3], np.int32), edge_T=p["edge_T"][:1])
    for batch in (False, True):
        for q in ({}, allc, noedge, dict(edge_i=rev["edge_i"], edge_j=rev["edge_j"], edge_T=rev["edge_T"]), repeated, skip,
                  dict(edge_sigma=np.full(6, 2.0))):
            rc, msg = _call(prob=q, batch=batch)
            assert rc == L.OV2_EINVAL and b"NULL context" in msg, msg


def test_apply_rejects_bad_arguments_without_a_gpu():
    from ov2slam_amd import _lib as L
    lib = _lib()
    I = np.array([0, 0, 0, 0, 0, 0, 1.0])
    win = np.tile(I, (3, 1)); young = np.tile(I, (2, 1)); X = np.zeros((4, 3)); kf = np.array([0, 1, 4, 2], np.int32)
    yn = np.full((2, 7), 7.0); Xo = np.full((4, 3), 7.0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(n_win=3, wo=win, wn=win, ini=I, new=I, n_young=2, yo=young, n_pts=4, xyz=X, k=kf, yn_=yn, xo=Xo):
        rc = lib.ov2_pose_graph_apply(None, n_win, vp(wo) if wo is not None else None, vp(wn), vp(ini), vp(new), n_young, vp(yo), vp(yn_), n_pts, vp(xyz),
                                      vp(k), vp(xo) if xo is not None else None)
        assert (yn == 7.0).all() and (Xo == 7.0).all(), "a rejected call wrote its outputs"
        return rc, lib.ov2_last_error()

    assert call()[1].endswith(b"NULL context")
    assert call(n_young=0, k=np.array([0, 1, 2, 2], np.int32))[1].endswith(b"NULL context")
    for kw, word in ((dict(n_win=-1), b"negative count"), (dict(wo=None), b"NULL win_old"), (dict(xo=None), b"NULL xyz"),
                     (dict(k=np.array([0, 1, 5, 2], np.int32)), b"pt_kf out of range"), (dict(k=np.array([0, -1, 1, 2], np.int32)), b"pt_kf out of range"),
                     (dict(wn=np.tile([0, 0, 0, 0, 0, 0, 0.0], (3, 1))), b"zero quaternion"), (dict(new=np.array([np.nan, 0, 0, 0, 0, 0, 1.0])), b"not finite"),
                     (dict(xyz=np.full((4, 3), np.inf)), b"xyz not finite"), (dict(n_win=0, n_young=0, wo=None), b"without a keyframe")):
        rc, msg = call(**kw)
        assert rc == L.OV2_EINVAL and word in msg and b"NULL context" not in msg, (kw, msg)


def test_capacity_constants_match_the_header():
    from ov2slam_amd import _lib as L
    assert L.OV2_PG_MAX_POSES == R.MAX_POSES == 16384 and L.OV2_PG_MAX_EDGES == R.MAX_EDGES == 32768
    hdr = open(os.path.join(ROOT, "include", "ov2slam_hip.h")).read()
    assert "#define OV2_PG_MAX_POSES %d" % L.OV2_PG_MAX_POSES in hdr and "#define OV2_PG_MAX_EDGES %d" % L.OV2_PG_MAX_EDGES in hdr
    assert (L.OV2_TERM_NO_CONVERGENCE, L.OV2_TERM_FUNCTION_TOL, L.OV2_TERM_PARAMETER_TOL, L.OV2_TERM_GRADIENT_TOL, L.OV2_TERM_MIN_RADIUS,
            L.OV2_TERM_INVALID_STEPS, L.OV2_TERM_FAILURE) == (R.TERM_NO_CONVERGENCE, R.TERM_FUNCTION_TOL, R.TERM_PARAMETER_TOL, R.TERM_GRADIENT_TOL,
                                                              R.TERM_MIN_RADIUS, R.TERM_INVALID_STEPS, R.TERM_FAILURE)
    # the capacity itself passes every input check: a chain of MAX_POSES poses with MAX_EDGES edges (every pair twice)
    n = R.MAX_POSES
    I = np.array([0, 0, 0, 0, 0, 0, 1.0])
    ei = np.concatenate([np.arange(n - 1), np.arange(n - 1), [0, 0]]).astype(np.int32)
    ej = np.concatenate([np.arange(1, n), np.arange(1, n), [1, 1]]).astype(np.int32)
    assert len(ei) == R.MAX_EDGES
    const = np.zeros(n, np.uint8); const[0] = 1
    rc, msg = _call(prob=dict(poses=np.tile(I, (n, 1)), pose_const=const, edge_i=ei, edge_j=ej, edge_T=np.tile(I, (len(ei), 1))))
    assert rc == L.OV2_EINVAL and b"NULL context" in msg
