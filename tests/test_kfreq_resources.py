"""k_fkf_parallax / k_fkf_sampson (ov2slam_amd/csrc/fkf.hip): a device-only compile for gfx950 shows no scratch and at most 128
VGPRs, and the C ABI of the frame-versus-keyframe passes rejects bad arguments and every class of malformed input without a GPU
(the inputs are checked before the context is touched) and writes nothing when it does."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import kfreq_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_k_fkf_kernels_use_no_scratch_and_128_vgprs(tmp_path):
    src = os.path.join(ROOT, "ov2slam_amd", "csrc", "fkf.hip")
    out = str(tmp_path / "fkf.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                    "--cuda-device-only", "-S", src, "-o", out], check=True, capture_output=True)
    txt = open(out).read()
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        res[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)\s", m.group(2))}
    names = [n for n in res if "k_fkf_" in n]
    assert len(names) == 2, names
    for n in names:
        print(n, "vgpr", res[n]["next_free_vgpr"], "sgpr", res[n]["next_free_sgpr"], "lds", res[n]["group_segment_fixed_size"])
        assert res[n]["private_segment_fixed_size"] == 0, (n, res[n])
        assert res[n]["next_free_vgpr"] <= 128, (n, res[n])
    lds = {n: res[n]["group_segment_fixed_size"] for n in names}
    assert max(lds.values()) <= 40 * 1024 and min(lds.values()) == 0, lds      # four work-groups of k_fkf_parallax per CU


def _lib():
    import ov2slam_amd
    return ov2slam_amd.load()


def test_abi_symbols_and_wrappers_exist():
    from ov2slam_amd import _lib as L
    from ov2slam_amd import keyframe as KF
    lib = _lib()
    for name in ("ov2_parallax", "ov2_parallax_batch", "ov2_kf_decision", "ov2_kf_decision_batch", "ov2_sampson_filter_2d",
                 "ov2_sampson_filter_2d_batch"):
        assert hasattr(lib, name), name
    for fn in (KF.parallax, KF.parallax_batch, KF.kf_decision, KF.kf_decision_batch, KF.sampson_filter_2d, KF.sampson_filter_2d_batch):
        assert callable(fn)
    assert (L.OV2_FKF_ALL, L.OV2_FKF_ONLY_2D, L.OV2_FKF_ONLY_3D, L.OV2_FKF_AVG, L.OV2_FKF_MEDIAN, L.OV2_FKF_AVG_WIDE) == \
        (R.ALL, R.ONLY_2D, R.ONLY_3D, R.AVG, R.MEDIAN, R.AVG_WIDE)
    assert (L.OV2_KF_C0, L.OV2_KF_C1, L.OV2_KF_C2, L.OV2_KF_CX, L.OV2_KF_RET_FEW_CELLS, L.OV2_KF_RET_FEW_3D, L.OV2_KF_RET_MANY_3D,
            L.OV2_KF_RET_TIME, L.OV2_KF_NONFINITE) == (R.C0, R.C1, R.C2, R.CX, R.RET_FEW_CELLS, R.RET_FEW_3D, R.RET_MANY_3D, R.RET_TIME,
                                                       R.NONFINITE)
    assert L.OV2_FKF_MAX_POINTS == 2048
    hdr = open(os.path.join(ROOT, "include", "ov2slam_hip.h")).read()
    assert "#define OV2_FKF_MAX_POINTS 2048" in hdr and "#define OV2_FKF_MAX_CELLS 65536" in hdr
    assert lib.ov2_version() == L.OV2_ABI_VERSION == 600


_SCENE = []


def _scene(n_cur=30, n_kf=25):
    if not _SCENE:
        P = R.make_params()
        _SCENE.append((P, R.flatten(*R.make_scene(P, np.random.default_rng(3), 30, 25))))
    P, item = _SCENE[0]
    item = dict(item)
    if (n_cur, n_kf) != (30, 25):
        item = R.flatten(*R.make_scene(P, np.random.default_rng(4), n_cur, n_kf))
    return P, item


ENTRIES = ["parallax", "parallax_batch", "decision", "decision_batch", "sampson", "sampson_batch"]
_POISON = 0x6E


def _call(entry, s, params=None, n_items=1, n_cur=None, null_result=None, F="ok"):
    """the entry point with a NULL context on the item struct `s`: (return code, message); the outputs must stay untouched"""
    from ov2slam_amd import _lib as L
    from ov2slam_amd import keyframe as KF
    lib = _lib()
    p = KF._as_fkf_params(params if params is not None else R.make_params())
    n = s.n_cur if n_cur is None else n_cur
    Fm = np.arange(9, dtype=np.float64)
    Fp = Fm.ctypes.data_as(C.POINTER(C.c_double)) if F == "ok" else None
    if entry.startswith("sampson"):
        r, out = KF._sampson_result(max(n, 1))
        for a in out.values():
            a.view(np.uint8)[...] = _POISON
        r.n_bad = 0x6E6E6E6E
        if null_result:
            setattr(r, null_result, None)
        rc = (lib.ov2_sampson_filter_2d_batch(None, n_items, C.byref(s), Fp, 3.0, C.byref(r)) if entry.endswith("batch") else
              lib.ov2_sampson_filter_2d(None, C.byref(s), Fp, 3.0, C.byref(r)))
        assert all((a.view(np.uint8) == _POISON).all() for a in out.values()) and r.n_bad == 0x6E6E6E6E, "a rejected call wrote its outputs"
    else:
        r = (L.KfDecisionResult if entry.startswith("decision") else L.ParallaxResult)()
        C.memset(C.byref(r), _POISON, C.sizeof(r))
        before = bytes(r)
        if entry == "parallax":
            rc = lib.ov2_parallax(None, C.byref(p), C.byref(s), 1, L.OV2_FKF_ALL, L.OV2_FKF_MEDIAN, C.byref(r))
        elif entry == "parallax_batch":
            rc = lib.ov2_parallax_batch(None, C.byref(p), n_items, C.byref(s), 1, L.OV2_FKF_ALL, L.OV2_FKF_MEDIAN, C.byref(r))
        elif entry == "decision":
            rc = lib.ov2_kf_decision(None, C.byref(p), C.byref(s), C.byref(r))
        else:
            rc = lib.ov2_kf_decision_batch(None, C.byref(p), n_items, C.byref(s), C.byref(r))
        assert bytes(r) == before, "a rejected call wrote its outputs"
    return rc, lib.ov2_last_error()


def _struct(item):
    from ov2slam_amd import keyframe as KF
    return KF._fkf_item(item)


@pytest.mark.parametrize("entry", ENTRIES)
def test_well_formed_input_reaches_the_context_check(entry):
    """the scene unmodified passes every input check: only the NULL context is left to object to"""
    from ov2slam_amd import _lib as L
    s, keep = _struct(_scene()[1])
    rc, msg = _call(entry, s)
    assert rc == L.OV2_EINVAL and b"NULL context" in msg, msg
    s, keep = _struct(_scene(0, 0)[1])                           # empty on both sides is well formed too
    rc, msg = _call(entry, s)
    assert rc == L.OV2_EINVAL and b"NULL context" in msg, msg


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_arguments_are_einval(entry):
    from ov2slam_amd import _lib as L
    lib = _lib()
    s, keep = _struct(_scene()[1])
    p = R.make_params()
    from ov2slam_amd import keyframe as KF
    pp = KF._as_fkf_params(p)
    r, rd = L.ParallaxResult(), L.KfDecisionResult()
    rs, out = KF._sampson_result(s.n_cur)
    F = np.zeros(9).ctypes.data_as(C.POINTER(C.c_double))
    calls = {
        "parallax": [lambda: lib.ov2_parallax(None, None, C.byref(s), 1, 0, 0, C.byref(r)), lambda: lib.ov2_parallax(None, C.byref(pp), None, 1, 0, 0, C.byref(r)),
                     lambda: lib.ov2_parallax(None, C.byref(pp), C.byref(s), 1, 0, 0, None)],
        "parallax_batch": [lambda: lib.ov2_parallax_batch(None, None, 1, C.byref(s), 1, 0, 0, C.byref(r)),
                           lambda: lib.ov2_parallax_batch(None, C.byref(pp), 1, None, 1, 0, 0, C.byref(r)),
                           lambda: lib.ov2_parallax_batch(None, C.byref(pp), 1, C.byref(s), 1, 0, 0, None)],
        "decision": [lambda: lib.ov2_kf_decision(None, None, C.byref(s), C.byref(rd)), lambda: lib.ov2_kf_decision(None, C.byref(pp), None, C.byref(rd)),
                     lambda: lib.ov2_kf_decision(None, C.byref(pp), C.byref(s), None)],
        "decision_batch": [lambda: lib.ov2_kf_decision_batch(None, None, 1, C.byref(s), C.byref(rd)),
                           lambda: lib.ov2_kf_decision_batch(None, C.byref(pp), 1, None, C.byref(rd)),
                           lambda: lib.ov2_kf_decision_batch(None, C.byref(pp), 1, C.byref(s), None)],
        "sampson": [lambda: lib.ov2_sampson_filter_2d(None, None, F, 3.0, C.byref(rs)), lambda: lib.ov2_sampson_filter_2d(None, C.byref(s), None, 3.0, C.byref(rs)),
                    lambda: lib.ov2_sampson_filter_2d(None, C.byref(s), F, 3.0, None)],
        "sampson_batch": [lambda: lib.ov2_sampson_filter_2d_batch(None, 1, None, F, 3.0, C.byref(rs)),
                          lambda: lib.ov2_sampson_filter_2d_batch(None, 1, C.byref(s), None, 3.0, C.byref(rs)),
                          lambda: lib.ov2_sampson_filter_2d_batch(None, 1, C.byref(s), F, 3.0, None)],
    }[entry]
    for f in calls:
        assert f() == L.OV2_EINVAL
        assert b"NULL" in lib.ov2_last_error() and b"NULL context" not in lib.ov2_last_error()
    if entry.endswith("batch"):
        rc, msg = _call(entry, s, n_items=-1)
        assert rc == L.OV2_EINVAL and b"n_items" in msg


_FULL_ONLY = ("cur_px", "cur_bv", "cur_Twc", "kf_Tcw")


@pytest.mark.parametrize("entry", ENTRIES)
def test_negative_counts_null_arrays_and_unsorted_ids(entry):
    from ov2slam_amd import _lib as L
    item = _scene()[1]
    for field in ("n_cur", "n_kf"):
        s, keep = _struct(item)
        setattr(s, field, -1)
        rc, msg = _call(entry, s, n_cur=30)
        assert rc == L.OV2_EINVAL and b"negative count" in msg, (field, msg)
    for field in ("cur_lmid", "cur_px", "cur_unpx", "cur_bv", "cur_is3d", "cur_Twc", "kf_lmid", "kf_unpx", "kf_Tcw"):
        s, keep = _struct(item)
        setattr(s, field, None)
        rc, msg = _call(entry, s)
        if entry.startswith("sampson") and field in _FULL_ONLY:          # not read by the Sampson pass
            assert rc == L.OV2_EINVAL and b"NULL context" in msg, (field, msg)
        else:
            assert rc == L.OV2_EINVAL and b"NULL" in msg and b"NULL context" not in msg, (field, msg)
    if entry.startswith("sampson"):
        for field in ("err", "bad"):
            s, keep = _struct(item)
            rc, msg = _call(entry, s, null_result=field)
            assert rc == L.OV2_EINVAL and b"result buffer" in msg, (field, msg)
    for name, edit in (("equal_neighbours", lambda a: a.__setitem__(7, a[6])), ("descending", lambda a: a.__setitem__(slice(None), a[::-1].copy())),
                       ("last_out_of_order", lambda a: a.__setitem__(len(a) - 1, a[0]))):
        s, keep = _struct(item)
        bad = np.array(item["kf_lmid"], np.int32)
        edit(bad)
        s.kf_lmid = bad.ctypes.data_as(C.POINTER(C.c_int))
        rc, msg = _call(entry, s)
        assert rc == L.OV2_EINVAL and b"unsorted" in msg, (name, msg)


@pytest.mark.parametrize("entry", ENTRIES)
def test_capacity_limits_are_eunsupported(entry):
    from ov2slam_amd import _lib as L
    item = _scene()[1]
    for field in ("n_cur", "n_kf"):
        s, keep = _struct(item)
        setattr(s, field, L.OV2_FKF_MAX_POINTS + 1)              # refused before any array is read
        rc, msg = _call(entry, s, n_cur=30)
        assert rc == L.OV2_EUNSUPPORTED and b"2048" in msg, (field, msg)
    if entry.endswith("batch"):
        s, keep = _struct(item)
        rc, msg = _call(entry, s, n_items=65536)
        assert rc == L.OV2_EUNSUPPORTED and b"65535" in msg


def test_bad_forms_and_grids():
    from ov2slam_amd import _lib as L
    from ov2slam_amd import keyframe as KF
    lib = _lib()
    P, item = _scene()
    s, keep = _struct(item)
    pp, r = KF._as_fkf_params(P), L.ParallaxResult()
    for unrot, filt, stat, word in ((2, 0, 0, b"unrot"), (-1, 0, 0, b"unrot"), (1, 3, 0, b"filter"), (1, -1, 0, b"filter"), (1, 0, 3, b"stat"),
                                    (1, 0, -1, b"stat")):
        assert lib.ov2_parallax(None, C.byref(pp), C.byref(s), unrot, filt, stat, C.byref(r)) == L.OV2_EINVAL
        assert word in lib.ov2_last_error()
    for kw in (dict(ncellsize=0), dict(nbwcells=0), dict(nbhcells=-3)):
        Pb = dict(P)
        Pb.update(kw)
        rc, msg = _call("decision", s, params=Pb)
        assert rc == L.OV2_EINVAL and b"not positive" in msg, (kw, msg)
        rc, msg = _call("parallax", s, params=Pb)                # the grid is the decision's only
        assert rc == L.OV2_EINVAL and b"NULL context" in msg, (kw, msg)
    Pb = dict(P)
    Pb.update(nbwcells=257, nbhcells=256)
    rc, msg = _call("decision_batch", s, params=Pb)
    assert rc == L.OV2_EUNSUPPORTED and b"65536" in msg
