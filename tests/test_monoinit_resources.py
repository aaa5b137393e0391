"""k_minit_gather / k_minit_decide and the lock-step form's k_minit_input / k_minit_apply (ov2slam_amd/csrc/monoinit.hip): a
device-only compile for gfx950 with the project's flags shows no scratch and no more LDS than the arrays the kernels declare; the
symbols and wrappers exist; the ctypes structs lay out like the
header's; and the C ABI rejects every class of malformed input without a GPU (the inputs are checked before the context is touched)
and writes nothing when it does."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import monoinit_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# k_minit_gather declares, per work-group: the distances (2048 doubles, 16384 B), the keyframe's ids / the draw's window (2048 ints,
# 8192 B), the keyframe slots (2048 shorts, 4096 B), the row starts (2048 / 8 unsigned shorts, 512 B) and eight control ints (32 B).
# k_minit_decide declares the removal flags (2048 bytes).  k_minit_input declares nothing; k_minit_apply the two sets of four
# per-wavefront counts of the compaction (res_rank).
LDS = dict(k_minit_gather=2048 * 8 + 2048 * 4 + 2048 * 2 + (2048 // 8) * 2 + 8 * 4, k_minit_decide=2048, k_minit_input=0,
           k_minit_apply=2 * 4 * 4)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_monoinit_kernels_use_no_scratch(tmp_path):
    src = os.path.join(ROOT, "ov2slam_amd", "csrc", "monoinit.hip")
    out = str(tmp_path / "monoinit.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                    "--cuda-device-only", "-S", src, "-o", out], check=True, capture_output=True)
    txt = open(out).read()
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        res[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)\s", m.group(2))}
    assert len(res) == len(LDS), sorted(res)
    assert LDS["k_minit_gather"] == 29216
    for want, lds in LDS.items():
        (n,) = [k for k in res if want in k]
        print(n, "vgpr", res[n]["next_free_vgpr"], "sgpr", res[n]["next_free_sgpr"], "lds", res[n]["group_segment_fixed_size"])
        assert res[n]["private_segment_fixed_size"] == 0, (n, res[n])
        assert res[n]["group_segment_fixed_size"] <= lds, (n, res[n])


def _lib():
    import ov2slam_amd
    return ov2slam_amd.load()


def test_abi_symbols_and_wrappers_exist():
    from ov2slam_amd import LockstepTracker, keyframe
    from ov2slam_amd import _lib as L
    lib = _lib()
    for name in ("ov2_mono_init", "ov2_mono_init_batch", "ov2_btracker_mono_init_begin", "ov2_btracker_mono_init_end", "ov2_btracker_mono_init"):
        assert hasattr(lib, name) and name in L.SIGNATURES, name
    for fn in (keyframe.mono_init, keyframe.mono_init_batch, keyframe.mono_init_params, LockstepTracker.monoInit,
               LockstepTracker.monoInitBegin, LockstepTracker.monoInitEnd):
        assert callable(fn)
    hdr = open(os.path.join(ROOT, "include", "ov2slam_hip.h")).read()
    names = ("RESET", "LOW_PARALLAX", "TOO_FEW_KPS", "TOO_FEW_MATCHES", "LOW_ROT_PARALLAX", "NO_MODEL", "READY", "NOT_REQUESTED", "NO_KEYFRAME")
    for k, nm in enumerate(names):
        assert re.search(r"OV2_MINIT_%s = %d\b" % (nm, k), hdr), nm
        assert getattr(keyframe, "MINIT_" + nm) == k and (k > R.READY or getattr(R, nm) == k)
    assert "NOT the reference's pose until a refinement exists" in hdr


def test_ctypes_structs_lay_out_like_the_header(tmp_path):
    from ov2slam_amd import _lib as L
    pairs = (("ov2_mono_init_params", L.MonoInitParams), ("ov2_mono_init_item", L.MonoInitItem), ("ov2_mono_init_result", L.MonoInitResult))
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
    assert L.MonoInitItem.fkf.offset == 0                        # ov2_parallax can be fed from the same item


# ---- argument checks with a NULL context --------------------------------------------------------------------------------------------
_POISON = 0x6E


def _scene():
    P, cur, kf = R.scene("quat_w")
    return P, R.flatten(cur, kf)


def _call(batch, *, P=None, item=None, n_items=1, edit=None, null=None):
    """the entry point with a NULL context: (return code, message).  edit(p, s, r): changes to the C structs before the call.  The
    outputs must stay as poisoned."""
    from ov2slam_amd import keyframe
    lib = _lib()
    P0, item0 = _scene()
    P = P0 if P is None else P
    item = item0 if item is None else item
    p = keyframe._as_mono_init_params(P)
    s, keep = keyframe._mono_init_item(item)
    n = s.fkf.n_cur
    outs = dict(removed=np.zeros(max(n, 1), np.uint8), pair_cur=np.zeros(max(n, 1), np.int32),
                samples=np.zeros((max(P["n_rows"], 1), 8), np.int32))
    r = keyframe.L.MonoInitResult()
    C.memset(C.byref(r), _POISON, C.sizeof(r))
    r.removed = outs["removed"].ctypes.data_as(C.POINTER(C.c_uint8))
    r.pair_cur = outs["pair_cur"].ctypes.data_as(C.POINTER(C.c_int))
    r.trace_samples = outs["samples"].ctypes.data_as(C.POINTER(C.c_int))
    for a in outs.values():
        a.view(np.uint8)[...] = _POISON
    if edit:
        edit(p, s, r)
    before = bytes(C.string_at(C.byref(r), C.sizeof(r)))
    pp, sp, rp = (None if null == "params" else C.byref(p)), (None if null == "item" else C.byref(s)), (None if null == "result" else C.byref(r))
    rc = lib.ov2_mono_init_batch(None, pp, n_items, sp, rp) if batch else lib.ov2_mono_init(None, pp, sp, rp)
    assert all((a.view(np.uint8) == _POISON).all() for a in outs.values()), "a rejected call wrote its output arrays"
    assert bytes(C.string_at(C.byref(r), C.sizeof(r))) == before, "a rejected call wrote its result"
    return rc, lib.ov2_last_error()


@pytest.mark.parametrize("batch", (False, True))
def test_well_formed_input_reaches_the_context_check(batch):
    from ov2slam_amd import _lib as L
    from tests import epifilter_ref as EF
    for name in ("quat_w", "n_cur_7", "n_kf_0", "nb2dkps_49", "size_308_rows_200"):
        P, cur, kf = R.scene(name)
        rc, msg = _call(batch, P=P, item=R.flatten(cur, kf))
        assert rc == L.OV2_EINVAL and b"NULL context" in msg, (name, msg)
    cur, kf = EF.geo_scene(71, 0, extra_kf=0)                                          # an empty frame against an empty keyframe
    rc, msg = _call(batch, item=R.flatten(cur, kf))
    assert rc == L.OV2_EINVAL and b"NULL context" in msg, msg
    if batch:
        rc, msg = _call(batch, n_items=0)
        assert rc == L.OV2_EINVAL and b"NULL context" in msg, msg


@pytest.mark.parametrize("batch", (False, True))
def test_null_arguments_counts_and_capacity_are_einval(batch):
    from ov2slam_amd import _lib as L
    for null in ("params", "item", "result"):
        rc, msg = _call(batch, null=null)
        assert rc == L.OV2_EINVAL and b"NULL" in msg and b"NULL context" not in msg, (null, msg)
    if batch:
        rc, msg = _call(batch, n_items=-1)
        assert rc == L.OV2_EINVAL and b"n_items" in msg
        rc, msg = _call(batch, n_items=65536)
        assert rc == L.OV2_EINVAL and b"65535" in msg
    for field in ("n_cur", "n_kf"):
        rc, msg = _call(batch, edit=lambda p, s, r, f=field: setattr(s.fkf, f, -1))
        assert rc == L.OV2_EINVAL and b"negative count" in msg, msg
        rc, msg = _call(batch, edit=lambda p, s, r, f=field: setattr(s.fkf, f, 2049))
        assert rc == L.OV2_EINVAL and b"2048" in msg, msg
    for field in ("cur_lmid", "cur_px", "cur_unpx", "cur_bv", "cur_is3d", "cur_Twc", "kf_lmid", "kf_unpx", "kf_Tcw"):
        rc, msg = _call(batch, edit=lambda p, s, r, f=field: setattr(s.fkf, f, None))
        assert rc == L.OV2_EINVAL and b"NULL" in msg and b"NULL context" not in msg, (field, msg)
    rc, msg = _call(batch, edit=lambda p, s, r: setattr(s, "kf_bv", None))
    assert rc == L.OV2_EINVAL and b"NULL kf_bv" in msg, msg
    rc, msg = _call(batch, edit=lambda p, s, r: setattr(r, "removed", None))
    assert rc == L.OV2_EINVAL and b"result buffer" in msg, msg
    # the optional outputs may be NULL
    rc, msg = _call(batch, edit=lambda p, s, r: (setattr(r, "pair_cur", None), setattr(r, "trace_samples", None)))
    assert rc == L.OV2_EINVAL and b"NULL context" in msg, msg
    P, item = _scene()
    lm = item["kf_lmid"].copy()
    lm[[3, 4]] = lm[[4, 3]]
    rc, msg = _call(batch, item=dict(item, kf_lmid=lm))
    assert rc == L.OV2_EINVAL and b"unsorted" in msg, msg


@pytest.mark.parametrize("batch", (False, True))
def test_non_finite_inputs_and_bad_params_are_einval(batch):
    from ov2slam_amd import _lib as L
    P, item = _scene()
    for field, idx in (("cur_bv", (4, 1)), ("kf_bv", (7, 2)), ("cur_Twc", (5,)), ("kf_Tcw", (1,))):
        for bad in (np.nan, np.inf):
            a = np.array(item[field], np.float64)
            a[idx] = bad
            rc, msg = _call(batch, item=dict(item, **{field: a}))
            assert rc == L.OV2_EINVAL and b"not finite" in msg, (field, msg)
    for kw, word in ((dict(threshold=0.0), b"threshold"), (dict(threshold=float("nan")), b"threshold"), (dict(max_iterations=-1), b"max_iterations"),
                     (dict(probability=1.0), b"probability"), (dict(probability=0.0), b"probability"), (dict(boptimize=True), b"boptimize"),
                     (dict(n_rows=-1), b"n_rows"), (dict(n_rows=4097), b"n_rows"), (dict(min_2d_kps=-1), b"min_2d_kps")):
        rc, msg = _call(batch, P=dict(P, **kw))
        assert rc == L.OV2_EINVAL and word in msg, (kw, msg)
    for bad in (np.nan, np.inf, -np.inf):
        rc, msg = _call(batch, P=dict(P, fkf=dict(P["fkf"], finit_parallax=bad)))
        assert rc == L.OV2_EINVAL and b"finit_parallax not finite" in msg, msg
    for bad in (np.nan, np.inf):
        K = list(P["fkf"]["K"])
        K[2] = bad
        rc, msg = _call(batch, P=dict(P, fkf=dict(P["fkf"], K=tuple(K))))
        assert rc == L.OV2_EINVAL and b"K not finite" in msg, msg
