"""k_pnp_solve / k_pose_gather / k_pose_decide (ov2slam_amd/csrc/pnp.hip): a device-only compile for gfx950 with the project's flags
shows no scratch; the symbols and wrappers of scope row f15 exist; the ctypes structs lay out like the header's; and the C ABI
rejects every class of malformed input without a GPU (the inputs are checked before the context is touched) and writes nothing
when it does."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import computepose_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_pnp_kernels_use_no_scratch(tmp_path):
    src = os.path.join(ROOT, "ov2slam_amd", "csrc", "pnp.hip")
    out = str(tmp_path / "pnp.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                    "--cuda-device-only", "-S", src, "-o", out], check=True, capture_output=True)
    txt = open(out).read()
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        res[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)\s", m.group(2))}
    assert len(res) == 3, sorted(res)
    for want in ("k_pnp_solve", "k_pose_gather", "k_pose_decide"):
        assert any(want in n for n in res), (want, sorted(res))
    for n in res:
        print(n, "vgpr", res[n]["next_free_vgpr"], "sgpr", res[n]["next_free_sgpr"], "lds", res[n]["group_segment_fixed_size"])
        assert res[n]["private_segment_fixed_size"] == 0, (n, res[n])
        assert res[n]["group_segment_fixed_size"] <= 8192, (n, res[n])       # the 2 KB mask, the partial sums, the control block
    assert not re.search(r"^\s+(global_atomic|flat_atomic|buffer_atomic|ds_add|ds_cmpst)", txt, re.M)     # fixed-order sums: no atomics


def _lib():
    import ov2slam_amd
    return ov2slam_amd.load()


def test_abi_symbols_and_wrappers_exist():
    from ov2slam_amd import _lib as L
    from ov2slam_amd import pose
    lib = _lib()
    for name in ("ov2_ceres_pnp", "ov2_ceres_pnp_batch", "ov2_compute_pose", "ov2_compute_pose_batch", "ov2_pose_from_model"):
        assert hasattr(lib, name) and name in L.SIGNATURES, name
    for fn in (pose.ceres_pnp, pose.ceres_pnp_batch, pose.compute_pose, pose.compute_pose_batch, pose.pose_from_model):
        assert callable(fn)
    assert lib.ov2_version() == L.OV2_ABI_VERSION == 600
    hdr = open(os.path.join(ROOT, "include", "ov2slam_hip.h")).read()
    assert "#define OV2_ABI_VERSION 600" in hdr
    assert "max_solver_time_in_seconds = 0.005 has no counterpart" in hdr
    assert (pose.TOO_FEW, pose.POSE_OK, pose.PNP_REQ_P3P, pose.P3P_RESET, pose.PNP_RESET, pose.PNP_KEEP) == \
           (R.TOO_FEW, R.POSE_OK, R.PNP_REQ_P3P, R.P3P_RESET, R.PNP_RESET, R.PNP_KEEP)
    for name in ("OV2_POSE_TOO_FEW = 0", "OV2_POSE_OK = 1", "OV2_POSE_PNP_REQ_P3P = 2", "OV2_POSE_P3P_RESET = 3", "OV2_POSE_PNP_RESET = 4",
                 "OV2_POSE_PNP_KEEP = 5"):
        assert name in hdr, name


def test_ctypes_structs_lay_out_like_the_header(tmp_path):
    from ov2slam_amd import _lib as L
    pairs = (("ov2_pnp_params", L.PnPParams), ("ov2_pnp_problem", L.PnPProblem), ("ov2_pnp_pass", L.PnPPass), ("ov2_pnp_result", L.PnPResult),
             ("ov2_pose_params", L.PoseParams), ("ov2_pose_problem", L.PoseProblem), ("ov2_pose_result", L.PoseResult))
    rename = {"passes": "pass"}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "ov2slam_hip.h"', "int main(void) {"]
    for cname, ct in pairs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in ct._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, rename.get(f, f)))
    lines += ["return 0; }"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for cname, ct in pairs:
        assert int(got[cname]) == C.sizeof(ct), cname
        for f, _ in ct._fields_:
            assert int(got["%s.%s" % (cname, f)]) == getattr(ct, f).offset, (cname, f)


def test_pose_from_model_matches_the_numpy_restatement_bit_for_bit():
    from ov2slam_amd import pose
    rng = np.random.default_rng(11)
    for k in range(200):
        Rm = R._so3_exp(rng.normal(0, 2.5 if k % 2 else 0.3, 3))
        m = np.concatenate([Rm.reshape(9), rng.normal(size=3)])
        assert np.array_equal(pose.pose_from_model(m).view(np.uint64), R.pose_from_model(m).view(np.uint64))


# ---- argument checks with a NULL context ------------------------------------------------------------------------------------------
_POISON = 0x6E
ENTRIES = ["pnp", "pnp_batch", "pose", "pose_batch"]


def _problem(n=30, do_p3p=True):
    return R.make_scene(3, n, outlier_frac=0.1, do_p3p=do_p3p)


def _call(entry, pb, params=None, n_items=1, edit=None, null=None):
    """the entry point with a NULL context: (return code, message).  edit(s, r): changes to the C structs before the call; null:
    'params' / 'problem' / 'result'.  The outputs must stay as poisoned."""
    from ov2slam_amd import pose
    lib = _lib()
    P = params if params is not None else R.params_of()
    pnp = entry.startswith("pnp")
    p = pose._as_pnp_params(P["pnp"]) if pnp else pose._as_pose_params(P)
    s, r, keep = (pose._pnp_problem if pnp else pose._pose_problem)(pb)
    outs = [keep["outliers" if pnp else "removed"]]
    C.memset(C.byref(r), _POISON, C.sizeof(r))
    if pnp:
        r.outliers = keep["outliers"].ctypes.data_as(C.POINTER(C.c_int))
    else:
        r.removed = keep["removed"].ctypes.data_as(C.POINTER(C.c_uint8))
    for a in outs:
        a.view(np.uint8)[...] = _POISON
    if edit:
        edit(s, r, p)
    before = bytes(C.string_at(C.byref(r), C.sizeof(r)))
    pp, sp, rp = (None if null == "params" else C.byref(p)), (None if null == "problem" else C.byref(s)), (None if null == "result" else C.byref(r))
    fn = getattr(lib, {"pnp": "ov2_ceres_pnp", "pnp_batch": "ov2_ceres_pnp_batch", "pose": "ov2_compute_pose",
                       "pose_batch": "ov2_compute_pose_batch"}[entry])
    rc = fn(None, pp, n_items, sp, rp) if entry.endswith("batch") else fn(None, pp, sp, rp)
    assert all((a.view(np.uint8) == _POISON).all() for a in outs), "a rejected call wrote its output arrays"
    assert bytes(C.string_at(C.byref(r), C.sizeof(r))) == before, "a rejected call wrote its result"
    return rc, lib.ov2_last_error()


@pytest.mark.parametrize("entry", ENTRIES)
def test_well_formed_input_reaches_the_context_check(entry):
    from ov2slam_amd import _lib as L
    for pb in (_problem(), _problem(0), _problem(3), _problem(30, do_p3p=False)):      # empty and tiny items are well formed too
        rc, msg = _call(entry, pb)
        assert rc == L.OV2_EINVAL and b"NULL context" in msg, msg
    if entry.endswith("batch"):
        rc, msg = _call(entry, _problem(), n_items=0)
        assert rc == L.OV2_EINVAL and b"NULL context" in msg, msg


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_arguments_and_negative_counts_are_einval(entry):
    from ov2slam_amd import _lib as L
    pb = _problem()
    for null in ("params", "problem", "result"):
        rc, msg = _call(entry, pb, null=null)
        assert rc == L.OV2_EINVAL and b"NULL" in msg and b"NULL context" not in msg, (null, msg)
    if entry.endswith("batch"):
        rc, msg = _call(entry, pb, n_items=-1)
        assert rc == L.OV2_EINVAL and b"n_items" in msg
        rc, msg = _call(entry, pb, n_items=65536)
        assert rc == L.OV2_EINVAL and b"65535" in msg

    def neg(s, r, p):
        s.n = -1
    rc, msg = _call(entry, pb, edit=neg)
    assert rc == L.OV2_EINVAL and b"negative count" in msg, msg
    fields = ("unpx", "wpt", "scale", "Twc") + (() if entry.startswith("pnp") else ("bv", "samples"))
    for field in fields:
        rc, msg = _call(entry, pb, edit=lambda s, r, p, f=field: setattr(s, f, None))
        assert rc == L.OV2_EINVAL and b"NULL" in msg and b"NULL context" not in msg, (field, msg)
    out = "outliers" if entry.startswith("pnp") else "removed"
    rc, msg = _call(entry, pb, edit=lambda s, r, p: setattr(r, out, None))
    assert rc == L.OV2_EINVAL and b"result buffer" in msg, msg
    if entry.startswith("pose"):
        def negrows(s, r, p):
            s.n_rows = -1
        rc, msg = _call(entry, pb, edit=negrows)
        assert rc == L.OV2_EINVAL and b"negative count" in msg, msg
        # bv and samples are not needed where the item does not search
        pb2 = _problem(30, do_p3p=False)
        rc, msg = _call(entry, pb2)
        assert rc == L.OV2_EINVAL and b"NULL context" in msg, msg


@pytest.mark.parametrize("entry", ENTRIES)
def test_non_finite_inputs_and_bad_params_are_einval(entry):
    from ov2slam_amd import _lib as L
    for field, shape_idx in (("unpx", (4, 1)), ("wpt", (7, 2)), ("Twc", (5,))) + (() if entry.startswith("pnp") else (("bv", (2, 0)),)):
        for bad in (np.nan, np.inf):
            pb = _problem()
            a = np.array(pb[field], np.float64)
            a[shape_idx] = bad
            rc, msg = _call(entry, dict(pb, **{field: a}))
            assert rc == L.OV2_EINVAL and b"not finite" in msg, (field, msg)
    pb = _problem()
    sc = pb["scale"].copy()
    sc[3] = 61
    rc, msg = _call(entry, dict(pb, scale=sc))
    assert rc == L.OV2_EINVAL and b"scale" in msg, msg
    P = R.params_of()
    for kw, word in ((dict(chi2th=0.0), b"chi2th"), (dict(chi2th=-1.0), b"chi2th"), (dict(chi2th=float("nan")), b"chi2th"),
                     (dict(nmaxiter=-1), b"nmaxiter"), (dict(K=np.array([np.nan, 1, 1, 1])), b"K not finite"),
                     (dict(K=np.array([0.0, 1, 1, 1])), b"fx / fy")):
        rc, msg = _call(entry, pb, params=dict(P, pnp=dict(P["pnp"], **kw)))
        assert rc == L.OV2_EINVAL and word in msg, (kw, msg)
    if entry.startswith("pose"):
        for kw, word in ((dict(threshold=0.0), b"threshold"), (dict(mode=7), b"mode"), (dict(max_iterations=-1), b"max_iterations"),
                         (dict(probability=1.0), b"probability"), (dict(boptimize=True), b"boptimize")):
            rc, msg = _call(entry, pb, params=dict(P, p3p=dict(P["p3p"], **kw)))
            assert rc == L.OV2_EINVAL and word in msg, (kw, msg)


@pytest.mark.parametrize("entry", ENTRIES)
def test_capacity_limits_are_einval(entry):
    from ov2slam_amd import _lib as L
    pb = R.make_scene(5, 2049, do_p3p=False)
    rc, msg = _call(entry, pb)
    assert rc == L.OV2_EINVAL and b"2048" in msg, msg
    if entry.startswith("pose"):
        pb = _problem()
        pb = dict(pb, samples=np.tile(pb["samples"], (103, 1))[:4097])
        rc, msg = _call(entry, pb)
        assert rc == L.OV2_EINVAL and b"4096" in msg, msg
