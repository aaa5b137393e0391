"""Scope row f16 without a GPU: the new symbols are in the header, the built library and the bindings; the ABI version is still 600;
the header still compiles as C and the new ctypes structs lay out like it; the kernels of csrc/framepose.hip use no scratch; and the
chain's kernels (pnp.hip, p3p.hip) report the resources DESIGN 4.10 / 4.19 give for the commit before this one."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NEW = ("ov2_btracker_track_frame_pose_begin", "ov2_btracker_track_frame_pose_end", "ov2_btracker_track_frame_pose",
       "ov2_btracker_last_pose_inputs")


def _resources(name):
    src = os.path.join(ROOT, "ov2slam_amd", "csrc", name + ".hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "--cuda-device-only",
                        "-S", src, "-o", "-"], check=True, capture_output=True, text=True)
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", r.stdout, re.S):
        res[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)\s", m.group(2))}
    return res, r.stdout


def _of(res, kernel):
    hits = [v for k, v in res.items() if kernel in k]
    assert len(hits) == 1, (kernel, sorted(res))
    return hits[0]


def test_symbols_bindings_and_abi_version():
    import ov2slam_amd
    from ov2slam_amd import _lib as L
    lib = ov2slam_amd.load()
    hdr = open(os.path.join(ROOT, "include", "ov2slam_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in L.SIGNATURES and name + "(" in hdr, name
    for name in ("trackFramePose", "trackFramePoseBegin", "trackFramePoseEnd", "lastPoseInputs"):
        assert callable(getattr(ov2slam_amd.LockstepTracker, name)), name
    assert lib.ov2_version() == L.OV2_ABI_VERSION == 600 and "#define OV2_ABI_VERSION 600" in hdr
    for words in ("IN SLOT SPACE", "33 % rule stays on the host", "CANNOT be checked on the host", "doepipolar: 1"):
        assert words in hdr, words


def test_header_compiles_as_c_and_the_new_structs_lay_out_like_it(tmp_path):
    from ov2slam_amd import _lib as L
    pairs = (("ov2_frame_pose_params", L.FramePoseParams), ("ov2_frame_pose_input", L.FramePoseInput))
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "ov2slam_hip.h"', "int main(void) {"]
    for cname, ct in pairs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in ct._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines += ["return 0; }"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for cname, ct in pairs:
        assert int(got[cname]) == C.sizeof(ct), cname
        for f, _ in ct._fields_:
            assert int(got["%s.%s" % (cname, f)]) == getattr(ct, f).offset, (cname, f)


def test_rejected_without_a_tracker():
    import ov2slam_amd
    from ov2slam_amd import _lib as L
    lib = ov2slam_amd.load()
    assert lib.ov2_btracker_track_frame_pose_begin(None, 1, None, 0, None, None, None, None, None, 1, None, None) == L.OV2_EINVAL
    assert lib.ov2_btracker_track_frame_pose_end(None, None, None, None, None) == L.OV2_EINVAL
    assert lib.ov2_btracker_last_pose_inputs(None, 0, None, None, None, None) == L.OV2_EINVAL


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_new_kernels_use_no_scratch():
    res, txt = _resources("framepose")
    assert len(res) == 3, sorted(res)
    for k in ("k_pose_select", "k_pose_pack", "k_pose_unpack"):
        r = _of(res, k)
        print(k, "vgpr", r["next_free_vgpr"], "sgpr", r["next_free_sgpr"], "lds", r["group_segment_fixed_size"])
        assert r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] == 0, (k, r)
        assert r["next_free_vgpr"] <= 64, (k, r)                 # eight wavefronts per SIMD stay possible
    assert not re.search(r"^\s+(global_atomic|flat_atomic|buffer_atomic|ds_add|ds_cmpst)", txt, re.M)


# (VGPRs, LDS bytes) of the commit before this one: DESIGN 4.19 (k_pnp_solve 224 / 3.8 KB, k_pose_gather 32 / 2 KB, k_pose_decide 10),
# DESIGN 4.10 (k_p3p_solve 194, no LDS) and that commit's own build for the two figures the document does not print
PARENT = {"pnp": {"k_pnp_solve": (224, 3848), "k_pose_gather": (32, 2048), "k_pose_decide": (10, 0)},
          "p3p": {"k_p3p_solve": (194, 0), "k_p3p_score": (54, 0), "k_p3p_pick": (80, 0)}}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("name", sorted(PARENT))
def test_chain_kernels_keep_their_resources(name):
    res, _ = _resources(name)
    assert len(res) == 3, sorted(res)
    for k, (vgpr, lds) in PARENT[name].items():
        r = _of(res, k)
        assert (r["next_free_vgpr"], r["group_segment_fixed_size"], r["private_segment_fixed_size"]) == (vgpr, lds, 0), (k, r)
