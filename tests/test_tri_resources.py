"""k_triangulate (ov2slam_amd/csrc/triangulate.hip): a device-only compile for gfx950 shows no scratch, and the C ABI of the
keyframe triangulation rejects bad arguments without a GPU (OV2_EINVAL before any device work)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_k_triangulate_uses_no_scratch(tmp_path):
    src = os.path.join(ROOT, "ov2slam_amd", "csrc", "triangulate.hip")
    out = str(tmp_path / "tri.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                    "--cuda-device-only", "-S", src, "-o", out], check=True, capture_output=True)
    txt = open(out).read()
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        res[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)\s", m.group(2))}
    names = [n for n in res if "k_triangulate" in n]
    assert len(names) == 1, names
    r = res[names[0]]
    assert r["private_segment_fixed_size"] == 0, r
    assert r["next_free_vgpr"] <= 128, r


def _lib():
    import ov2slam_amd
    return ov2slam_amd.load()


def test_null_context_is_einval():
    from ov2slam_amd import _lib as L
    lib = _lib()
    p, k, r = L.TriParams(), L.TriKeyframe(), L.TriResult()
    assert lib.ov2_triangulate_keyframe(None, C.byref(p), C.byref(k), C.byref(r)) == L.OV2_EINVAL
    assert lib.ov2_triangulate_keyframe_batch(None, C.byref(p), 1, C.byref(k), C.byref(r)) == L.OV2_EINVAL
    assert lib.ov2_triangulate_keyframe(None, None, None, None) == L.OV2_EINVAL
    assert b"NULL" in lib.ov2_last_error()
