"""k_prior_frame / k_prior_stereo (ov2slam_amd/csrc/priors.hip): a device-only compile for gfx950 shows no scratch, no LDS and at
most 128 VGPRs; the ctypes structs lay out like the header's; and the C ABI of the tracking priors rejects bad arguments and every
class of malformed input without a GPU (the inputs are checked before the context is touched) and writes nothing when it does."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import priors_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_k_prior_kernels_use_no_scratch_and_128_vgprs(tmp_path):
    src = os.path.join(ROOT, "ov2slam_amd", "csrc", "priors.hip")
    out = str(tmp_path / "priors.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                    "--cuda-device-only", "-S", src, "-o", out], check=True, capture_output=True)
    txt = open(out).read()
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        res[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)\s", m.group(2))}
    assert len(res) == 2, sorted(res)                                # exactly the two kernels
    names = [n for n in res if "k_prior_" in n]
    assert len(names) == 2 and any("k_prior_frame" in n for n in names) and any("k_prior_stereo" in n for n in names), names
    for n in names:
        print(n, "vgpr", res[n]["next_free_vgpr"], "sgpr", res[n]["next_free_sgpr"], "lds", res[n]["group_segment_fixed_size"])
        assert res[n]["private_segment_fixed_size"] == 0, (n, res[n])
        assert res[n]["next_free_vgpr"] <= 128, (n, res[n])
        assert res[n]["group_segment_fixed_size"] == 0, (n, res[n])
    assert not re.search(r"^\s+(global_atomic|flat_atomic|buffer_atomic|ds_)", txt, re.M)        # no atomics, no LDS traffic


def _lib():
    import ov2slam_amd
    return ov2slam_amd.load()


def test_abi_symbols_and_wrappers_exist():
    from ov2slam_amd import _lib as L
    from ov2slam_amd import frontend, priors
    lib = _lib()
    for name in ("ov2_klt_priors", "ov2_klt_priors_batch", "ov2_stereo_priors", "ov2_stereo_priors_batch",
                 "ov2_btracker_track_frame_map_begin", "ov2_btracker_track_frame_map", "ov2_btracker_last_priors"):
        assert hasattr(lib, name) and name in L.SIGNATURES, name
    for fn in (priors.klt_priors, priors.klt_priors_batch, priors.stereo_priors, priors.stereo_priors_batch,
               frontend.LockstepTracker.trackFrameMap, frontend.LockstepTracker.track_frame_map,
               frontend.LockstepTracker.trackFrameMapBegin, frontend.LockstepTracker.lastPriors):
        assert callable(fn)
    assert lib.ov2_version() == L.OV2_ABI_VERSION == 600
    hdr = open(os.path.join(ROOT, "include", "ov2slam_hip.h")).read()
    assert "#define OV2_ABI_VERSION 600" in hdr
    assert "priors3d_h and has_prior3d_h: non-zero means a prior" in hdr      # the contract with ov2_stereo_match is written down


def test_ctypes_structs_lay_out_like_the_header(tmp_path):
    from ov2slam_amd import _lib as L
    pairs = (("ov2_klt_priors_params", L.KltPriorsParams), ("ov2_klt_priors_item", L.KltPriorsItem),
             ("ov2_klt_priors_result", L.KltPriorsResult), ("ov2_stereo_priors_params", L.StereoPriorsParams),
             ("ov2_stereo_priors_item", L.StereoPriorsItem), ("ov2_stereo_priors_result", L.StereoPriorsResult))
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "ov2slam_hip.h"', "int main(void) {"]
    for cname, ct in pairs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in ct._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
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


_SCENE = {}
_POISON = 0x6E
ENTRIES = ["klt", "klt_batch", "stereo", "stereo_batch"]


def _scene(n=30):
    if n not in _SCENE:
        P = R.make_params(D=R.RADTAN4)
        frame, mps = R.make_scene(P, np.random.default_rng(3), n)
        _SCENE[n] = (P, R.flatten(P, frame, mps))
    return _SCENE[n]


def _struct(entry, item):
    from ov2slam_amd import priors
    return priors._klt_item(item) if entry.startswith("klt") else priors._stereo_item(item)


def _call(entry, s, params=None, n_items=1, n=None, null_result=None, null_params=False, null_item=False, null_res=False):
    """the entry point with a NULL context on the item struct `s`: (return code, message); the outputs must stay untouched"""
    from ov2slam_amd import priors
    lib = _lib()
    P = params if params is not None else _scene()[0]
    klt = entry.startswith("klt")
    p = priors._as_klt_params(P) if klt else priors._as_stereo_params(P)
    r, out = (priors._klt_result if klt else priors._stereo_result)(max(s.n if n is None else n, 1))
    for a in out.values():
        a.view(np.uint8)[...] = _POISON
    counts = [f for f, _ in type(r)._fields_ if f.startswith("n_")]
    for f in counts:
        setattr(r, f, 0x6E6E6E6E)
    if null_result:
        setattr(r, null_result, None)
    pp, sp, rp = (None if null_params else C.byref(p)), (None if null_item else C.byref(s)), (None if null_res else C.byref(r))
    fn = getattr(lib, {"klt": "ov2_klt_priors", "klt_batch": "ov2_klt_priors_batch", "stereo": "ov2_stereo_priors",
                       "stereo_batch": "ov2_stereo_priors_batch"}[entry])
    rc = fn(None, pp, n_items, sp, rp) if entry.endswith("batch") else fn(None, pp, sp, rp)
    assert all((a.view(np.uint8) == _POISON).all() for a in out.values()), "a rejected call wrote its outputs"
    assert all(getattr(r, f) == 0x6E6E6E6E for f in counts), "a rejected call wrote its counts"
    return rc, lib.ov2_last_error()


@pytest.mark.parametrize("entry", ENTRIES)
def test_well_formed_input_reaches_the_context_check(entry):
    """the scene unmodified passes every input check: only the NULL context is left to object to"""
    from ov2slam_amd import _lib as L
    for n in (30, 0):                                            # an item without keypoints is well formed too
        s, keep = _struct(entry, _scene(n)[1])
        rc, msg = _call(entry, s)
        assert rc == L.OV2_EINVAL and b"NULL context" in msg, msg
    if entry.startswith("stereo"):                               # rectified: the cell tables are not needed
        s, keep = _struct(entry, _scene()[1])
        s.cell_start, s.cell_kp = None, None
        rc, msg = _call(entry, s, params=dict(_scene()[0], rect=True))
        assert rc == L.OV2_EINVAL and b"NULL context" in msg, msg


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_arguments_and_negative_counts_are_einval(entry):
    from ov2slam_amd import _lib as L
    s, keep = _struct(entry, _scene()[1])
    for kw in (dict(null_params=True), dict(null_item=True), dict(null_res=True)):
        rc, msg = _call(entry, s, **kw)
        assert rc == L.OV2_EINVAL and b"NULL" in msg and b"NULL context" not in msg, (kw, msg)
    if entry.endswith("batch"):
        rc, msg = _call(entry, s, n_items=-1)
        assert rc == L.OV2_EINVAL and b"n_items" in msg
    s, keep = _struct(entry, _scene()[1])
    s.n = -1
    rc, msg = _call(entry, s, n=30)
    assert rc == L.OV2_EINVAL and b"negative count" in msg, msg
    fields = ("Tcw", "px", "is3d", "wpt") if entry.startswith("klt") else ("Tcw", "px", "unpx", "bv", "wpt", "state", "cell_start", "cell_kp")
    for field in fields:
        s, keep = _struct(entry, _scene()[1])
        setattr(s, field, None)
        rc, msg = _call(entry, s)
        assert rc == L.OV2_EINVAL and b"NULL" in msg and b"NULL context" not in msg, (field, msg)
    for field in ("prior", "has_prior") + (() if entry.startswith("klt") else ("skip",)):
        s, keep = _struct(entry, _scene()[1])
        rc, msg = _call(entry, s, null_result=field)
        assert rc == L.OV2_EINVAL and b"result buffer" in msg, (field, msg)


@pytest.mark.parametrize("entry", ENTRIES)
def test_bad_camera_is_rejected(entry):
    from ov2slam_amd import _lib as L
    P, item = _scene()
    s, keep = _struct(entry, item)
    for kw in (dict(img_w=0), dict(img_h=-480), dict(img_w=float("nan"))):
        rc, msg = _call(entry, s, params=dict(P, **kw))
        assert rc == L.OV2_EINVAL and b"not positive" in msg, (kw, msg)
    rc, msg = _call(entry, s, params=dict(P, model=7))
    assert rc == L.OV2_EINVAL and b"camera model" in msg, msg
    for model, Dv in (("pinhole", (0.1, 0.2, 0.3)), ("pinhole", (0.1,) * 6), ("pinhole", (0.1,) * 14), ("fisheye", (0.1,) * 5),
                      ("fisheye", (0.1,) * 8)):
        rc, msg = _call(entry, s, params=dict(P, model=model, D=Dv))
        assert rc == L.OV2_EUNSUPPORTED and b"coefficient count" in msg, (model, len(Dv), msg)
    for model, Dv in (("pinhole", None), ("pinhole", (0.1,) * 5), ("pinhole", (0.1,) * 8), ("pinhole", (0.1,) * 12), ("fisheye", None),
                      ("fisheye", (0.1,) * 4)):
        rc, msg = _call(entry, s, params=dict(P, model=model, D=Dv))
        assert rc == L.OV2_EINVAL and b"NULL context" in msg, (model, Dv, msg)
    if entry.startswith("stereo"):
        for c in (0, -35):
            rc, msg = _call(entry, s, params=dict(P, ncellsize=c))
            assert rc == L.OV2_EINVAL and b"ncellsize" in msg, msg


@pytest.mark.parametrize("entry", ["stereo", "stereo_batch"])
def test_malformed_tables_and_states_are_einval(entry):
    from ov2slam_amd import _lib as L
    P, item = _scene()
    n = len(item["state"])
    ncells = len(item["cell_start"]) - 1

    def with_(field, edit):
        a = np.array(item[field])
        edit(a)
        return dict(item, **{field: a})

    for name, bad, word in (
            ("state_3", with_("state", lambda a: a.__setitem__(5, 3)), b"state > 2"),
            ("state_255", with_("state", lambda a: a.__setitem__(n - 1, 255)), b"state > 2"),
            ("cell_kp_minus_one", with_("cell_kp", lambda a: a.__setitem__(0, -1)), b"outside the keypoint table"),
            ("cell_kp_n", with_("cell_kp", lambda a: a.__setitem__(len(a) - 1, n)), b"outside the keypoint table"),
            ("offsets_start_at_1", with_("cell_start", lambda a: a.__setitem__(0, 1)), b"does not start at 0"),
            ("offsets_decrease", with_("cell_start", lambda a: a.__setitem__(ncells // 2, a[-1] + 1)), b"decreases")):
        from ov2slam_amd import priors
        s, keep = priors._item(bad, L.StereoPriorsItem, priors._STEREO_FIELDS, "stereo_priors")
        cs, ck = np.ascontiguousarray(bad["cell_start"], np.int32), np.ascontiguousarray(bad["cell_kp"], np.int32)
        s.cell_start, s.cell_kp = cs.ctypes.data_as(C.POINTER(C.c_int)), ck.ctypes.data_as(C.POINTER(C.c_int))
        rc, msg = _call(entry, s)
        assert rc == L.OV2_EINVAL and word in msg, (name, msg)


@pytest.mark.parametrize("entry", ENTRIES)
def test_capacity_limits_are_eunsupported(entry):
    """more than 65535 items, and more than 2^31 - 1 keypoints in one call: both refused from the counts alone, before any array of
    the items is read (the items of the second case all point at the same small arrays)"""
    from ov2slam_amd import _lib as L
    from ov2slam_amd import priors
    if not entry.endswith("batch"):
        return
    lib = _lib()
    s, keep = _struct(entry, _scene()[1])
    rc, msg = _call(entry, s, n_items=65536)
    assert rc == L.OV2_EUNSUPPORTED and b"65535" in msg
    klt = entry.startswith("klt")
    B = 65535
    S = ((L.KltPriorsItem if klt else L.StereoPriorsItem) * B)()
    for b in range(B):
        C.memmove(C.byref(S[b]), C.byref(s), C.sizeof(s))
        S[b].n = 40000                                           # 65535 x 40000 > 2^31 - 1
    R_ = ((L.KltPriorsResult if klt else L.StereoPriorsResult) * B)()
    p = priors._as_klt_params(_scene()[0]) if klt else priors._as_stereo_params(_scene()[0])
    fn = lib.ov2_klt_priors_batch if klt else lib.ov2_stereo_priors_batch
    rc = fn(None, C.byref(p), B, S, R_)
    assert rc == L.OV2_EUNSUPPORTED and b"2^31 - 1" in lib.ov2_last_error(), lib.ov2_last_error()


def test_lockstep_map_form_rejects_a_null_tracker_without_a_gpu():
    from ov2slam_amd import _lib as L
    lib = _lib()
    assert lib.ov2_btracker_track_frame_map(None, 1, None, 0, None, None, None, None, None, 1, None, None, None) == L.OV2_EINVAL
    assert lib.ov2_btracker_track_frame_map_begin(None, 1, None, 0, None, None, None, None, None, 1) == L.OV2_EINVAL
    assert lib.ov2_btracker_last_priors(None, 0, 0, None, None) == L.OV2_EINVAL
