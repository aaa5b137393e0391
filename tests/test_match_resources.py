"""k_map_match<false / true> / k_map_pick (ov2slam_amd/csrc/mapmatch.hip): a device-only compile for gfx950 shows no scratch, no LDS,
at most 128 VGPRs (four wavefronts per SIMD) and no more VGPRs per instantiation than the mapper's and the loop closer's kernels took
as separate files, and the C ABI of the local-map matching rejects bad arguments and every class of malformed input
without a GPU (the inputs are checked before the context is touched)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import match_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_k_map_kernels_use_no_scratch_no_lds_and_their_vgpr_budgets(tmp_path):
    src = os.path.join(ROOT, "ov2slam_amd", "csrc", "mapmatch.hip")
    out = str(tmp_path / "mapmatch.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                    "--cuda-device-only", "-S", src, "-o", out], check=True, capture_output=True)
    txt = open(out).read()
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        res[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)\s", m.group(2))}
    # exactly three kernels: the two instantiations of k_map_match (Itanium mangling: ILb0E = <false>, ILb1E = <true>) and k_map_pick
    assert len(res) == 3, sorted(res)
    mapper = [n for n in res if "k_map_match" in n and "ILb0E" in n]
    loop = [n for n in res if "k_map_match" in n and "ILb1E" in n]
    pick = [n for n in res if "k_map_pick" in n]
    assert len(mapper) == len(loop) == len(pick) == 1, sorted(res)
    for n in res:
        print(n, "vgpr", res[n]["next_free_vgpr"], "sgpr", res[n]["next_free_sgpr"], "lds", res[n]["group_segment_fixed_size"])
        assert res[n]["private_segment_fixed_size"] == 0, (n, res[n])
        assert res[n]["group_segment_fixed_size"] == 0, (n, res[n])
        assert res[n]["next_free_vgpr"] <= 128, (n, res[n])
    assert res[mapper[0]]["next_free_vgpr"] <= 115, res[mapper[0]]       # what the mapper's kernel took in a file of its own
    assert res[loop[0]]["next_free_vgpr"] <= 72, res[loop[0]]            # what the loop closer's kernel took in a file of its own


def _lib():
    import ov2slam_amd
    return ov2slam_amd.load()


def test_null_arguments_are_einval():
    from ov2slam_amd import _lib as L
    lib = _lib()
    p, k, r = L.MatchParams(), L.MatchKeyframe(), L.MatchResult()
    assert lib.ov2_match_to_map(None, None, None, None) == L.OV2_EINVAL
    assert b"NULL" in lib.ov2_last_error()
    assert lib.ov2_match_to_map(None, C.byref(p), None, C.byref(r)) == L.OV2_EINVAL
    assert lib.ov2_match_to_map_batch(None, None, 1, C.byref(k), C.byref(r)) == L.OV2_EINVAL
    assert b"NULL" in lib.ov2_last_error()
    assert lib.ov2_match_to_map_batch(None, C.byref(_params()), 1, None, None) == L.OV2_EINVAL
    assert lib.ov2_match_to_map_batch(None, C.byref(_params()), -1, C.byref(k), C.byref(r)) == L.OV2_EINVAL
    assert b"n_items" in lib.ov2_last_error()


def _params(**kw):
    from ov2slam_amd import mapper
    P = R.make_params()
    P.update(kw)
    return mapper._as_match_params(P)


def _scene():
    M = R.make_scene(R.make_params(), np.random.default_rng(3), n_kp=30, n_lm=40)
    return R.flatten(M)[0]


def _call(kf, params=None, batch=False, n_items=1):
    """the call with a NULL context: (return code, message, the result arrays)"""
    from ov2slam_amd import mapper
    lib = _lib()
    s, keep, n_lm, n_kp = mapper._match_keyframe(kf)
    r, out = mapper._match_result(n_lm, n_kp)
    for a in out.values():
        a.view(np.uint8)[...] = 0xEE
    p = params if params is not None else _params()
    if batch:
        rc = lib.ov2_match_to_map_batch(None, C.byref(p), n_items, C.byref(s), C.byref(r))
    else:
        rc = lib.ov2_match_to_map(None, C.byref(p), C.byref(s), C.byref(r))
    assert all((a.view(np.uint8) == 0xEE).all() for a in out.values()), "a rejected call wrote its outputs"
    return rc, lib.ov2_last_error()


def test_well_formed_input_reaches_the_context_check():
    """the same scene unmodified passes every input check: only the NULL context is left to object to"""
    from ov2slam_amd import _lib as L
    for batch in (False, True):
        rc, msg = _call(_scene(), batch=batch)
        assert rc == L.OV2_EINVAL and b"NULL context" in msg, msg


def _mod(kf, name, fn):
    kf = dict(kf)
    a = np.array(kf[name])
    fn(a)
    kf[name] = a
    return kf


def _first_row_with_two_obs(kf):
    n = np.diff(kf["obs_start"])
    return int(np.nonzero(n >= 2)[0][0])


MALFORMED = [
    ("kp_mp_above_table", lambda kf: _mod(kf, "kp_mp", lambda a: a.__setitem__(0, len(kf["obs_start"]) - 1)), b"kp_mp"),
    ("kp_mp_below_minus_one", lambda kf: _mod(kf, "kp_mp", lambda a: a.__setitem__(0, -2)), b"kp_mp"),
    ("lm_mp_outside", lambda kf: _mod(kf, "lm_mp", lambda a: a.__setitem__(0, len(kf["obs_start"]) - 1)), b"lm_mp"),
    ("lm_mp_negative", lambda kf: _mod(kf, "lm_mp", lambda a: a.__setitem__(0, -1)), b"lm_mp"),
    ("obs_kf_outside", lambda kf: _mod(kf, "obs_kf", lambda a: a.__setitem__(0, len(kf["kf_Tcw"]))), b"obs_kf"),
    ("cell_kp_outside", lambda kf: _mod(kf, "cell_kp", lambda a: a.__setitem__(0, len(kf["kp_mp"]))), b"cell_kp"),
    ("cell_kp_negative", lambda kf: _mod(kf, "cell_kp", lambda a: a.__setitem__(0, -1)), b"cell_kp"),
    ("obs_kfid_unsorted", lambda kf: _mod(kf, "obs_kfid", lambda a: a.__setitem__(kf["obs_start"][_first_row_with_two_obs(kf)] + 1,
                                                                                   a[kf["obs_start"][_first_row_with_two_obs(kf)]])), b"unsorted"),
    ("obs_start_decreases", lambda kf: _mod(kf, "obs_start", lambda a: a.__setitem__(1, a[2] + 1)), b"obs_start"),
    ("desc_start_decreases", lambda kf: _mod(kf, "desc_start", lambda a: a.__setitem__(1, a[2] + 1)), b"desc_start"),
    ("cell_start_decreases", lambda kf: _mod(kf, "cell_start", lambda a: a.__setitem__(1, a[-1] + 1)), b"cell_start"),
    ("obs_start_not_from_zero", lambda kf: _mod(kf, "obs_start", lambda a: a.__setitem__(0, -1)), b"obs_start"),
    ("cell_start_not_from_zero", lambda kf: _mod(kf, "cell_start", lambda a: a.__setitem__(0, 1)), b"cell_start"),
]


@pytest.mark.parametrize("batch", [False, True], ids=["single", "batch"])
@pytest.mark.parametrize("case", MALFORMED, ids=lambda c: c[0])
def test_malformed_input_is_rejected_without_a_gpu(case, batch):
    from ov2slam_amd import _lib as L
    from ov2slam_amd import mapper
    name, make, word = case
    kf = make(_scene())
    lib = _lib()
    # around the Python wrapper's own length checks: build the struct from the valid scene, then point it at the bad array
    good = _scene()
    s, keep, n_lm, n_kp = mapper._match_keyframe(good)
    bad = {}
    for f, dt, ct in mapper._MATCH_FIELDS:
        if not np.array_equal(kf[f], good[f]):
            bad[f] = np.ascontiguousarray(kf[f], dtype=dt)
            setattr(s, f, bad[f].ctypes.data_as(C.POINTER(ct)))
    assert len(bad) == 1, (name, list(bad))
    r, out = mapper._match_result(n_lm, n_kp)
    for a in out.values():
        a.view(np.uint8)[...] = 0xEE
    p = _params()
    if batch:
        rc = lib.ov2_match_to_map_batch(None, C.byref(p), 1, C.byref(s), C.byref(r))
    else:
        rc = lib.ov2_match_to_map(None, C.byref(p), C.byref(s), C.byref(r))
    msg = lib.ov2_last_error()
    assert rc == L.OV2_EINVAL and word in msg and b"NULL context" not in msg, (name, rc, msg)
    assert all((a.view(np.uint8) == 0xEE).all() for a in out.values()), "a rejected call wrote its outputs"


def test_negative_counts_and_null_arrays():
    from ov2slam_amd import _lib as L
    from ov2slam_amd import mapper
    lib = _lib()
    kf = _scene()
    for field in ("n_kp", "n_mp", "n_kf", "n_lm"):
        s, keep, n_lm, n_kp = mapper._match_keyframe(kf)
        setattr(s, field, -1)
        r, out = mapper._match_result(n_lm, n_kp)
        assert lib.ov2_match_to_map(None, C.byref(_params()), C.byref(s), C.byref(r)) == L.OV2_EINVAL
        assert b"negative count" in lib.ov2_last_error()
    for field in ("Tcw", "kp_px", "kp_mp", "cell_start", "cell_kp", "obs_start", "obs_kfid", "obs_kf", "obs_px", "desc_start", "desc", "kf_Tcw",
                  "lm_mp", "lm_wpt"):
        s, keep, n_lm, n_kp = mapper._match_keyframe(kf)
        setattr(s, field, None)
        r, out = mapper._match_result(n_lm, n_kp)
        assert lib.ov2_match_to_map(None, C.byref(_params()), C.byref(s), C.byref(r)) == L.OV2_EINVAL, field
        assert b"NULL" in lib.ov2_last_error() and b"NULL context" not in lib.ov2_last_error(), field
    for field in ("lm_status", "lm_kp", "lm_dist", "lm_projpx", "kp_lm", "kp_dist"):
        s, keep, n_lm, n_kp = mapper._match_keyframe(kf)
        r, out = mapper._match_result(n_lm, n_kp)
        setattr(r, field, None)
        assert lib.ov2_match_to_map(None, C.byref(_params()), C.byref(s), C.byref(r)) == L.OV2_EINVAL, field
        assert b"result buffer" in lib.ov2_last_error(), field


def test_unsupported_parameters():
    from ov2slam_amd import _lib as L
    kf = _scene()
    for kw in (dict(D=(0.1, 0.01, 0.001)), dict(D=(0.1,) * 6), dict(D=(0.1,) * 14), dict(D=(0.1,) * 5, model="fisheye"),
               dict(desc_bytes=64), dict(desc_bytes=16)):
        rc, msg = _call(kf, params=_params(**kw))
        assert rc == L.OV2_EUNSUPPORTED and msg, (kw, msg)
    rc, msg = _call(kf, batch=True, n_items=65536)
    assert rc == L.OV2_EUNSUPPORTED and b"65535" in msg
    for kw in (dict(ncellsize=0), dict(img_w=0), dict(img_h=-480)):
        rc, msg = _call(kf, params=_params(**kw))
        assert rc == L.OV2_EINVAL and b"not positive" in msg, (kw, msg)
