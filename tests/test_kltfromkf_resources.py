"""The from-keyframe tracking kernels (k_track_klt_kf_w in ov2slam_amd/csrc/lkw_kf.hip, k_track_klt_kf<9> in lk.hip) cost no more
than their siblings k_track_klt_w / k_track_klt<9>: no scratch, no more LDS, and no more VGPRs than the sibling plus the two that
hold the one extra float2 (retry_prior).  The siblings themselves keep the figures they had before the from-keyframe kernels were
added (a device-only compile of that tree for gfx950 with these flags): adding a kernel to a translation unit can move the register
allocation of the kernels already in it, which is why k_track_klt_kf_w has a file of its own.  Kernel metadata only; no GPU needed,
skipped without hipcc."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

FLOAT2_VGPRS = 2

# (next_free_vgpr, group_segment_fixed_size, private_segment_fixed_size) of the siblings before this feature: <FACC = true>, <false>
BEFORE = {
    "k_track_klt_w": {True: (113, 1600, 0), False: (103, 928, 0)},
    "k_track_klt<9>": {True: (125, 0, 0), False: (119, 0, 0)},
}


def kernel_resources(tmp_path, name):
    src = os.path.join(ROOT, "ov2slam_amd", "csrc", name)
    out = str(tmp_path / (name + ".s"))
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                    "--cuda-device-only", "-S", src, "-o", out], check=True, capture_output=True)
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", open(out).read(), re.S):
        res[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)\s", m.group(2))}
    return res


def figures(res, mangled_prefix, facc):
    """the one kernel whose mangled name starts with the prefix and carries the FACC template argument"""
    names = [n for n in res if n.startswith(mangled_prefix) and ("Lb1E" if facc else "Lb0E") in n]
    assert len(names) == 1, (mangled_prefix, facc, names)
    r = res[names[0]]
    return r["next_free_vgpr"], r["group_segment_fixed_size"], r["private_segment_fixed_size"]


def check_pair(new, old, before):
    assert old == before, "the sibling changed: %r, was %r" % (old, before)
    assert new[2] == 0, "scratch: %d bytes" % new[2]
    assert new[1] <= old[1], "LDS: %d > %d" % (new[1], old[1])
    assert new[0] <= old[0] + FLOAT2_VGPRS, "VGPRs: %d > %d + %d" % (new[0], old[0], FLOAT2_VGPRS)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("facc", [False, True])
def test_wave_kernel_costs_no_more_than_k_track_klt_w(tmp_path, facc):
    old = figures(kernel_resources(tmp_path, "lkw.hip"), "_Z13k_track_klt_wIL", facc)
    new = figures(kernel_resources(tmp_path, "lkw_kf.hip"), "_Z16k_track_klt_kf_wIL", facc)
    check_pair(new, old, BEFORE["k_track_klt_w"][facc])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("facc", [False, True])
def test_row_kernel_costs_no_more_than_k_track_klt(tmp_path, facc):
    res = kernel_resources(tmp_path, "lk.hip")
    old = figures(res, "_Z11k_track_kltILi9E", facc)
    new = figures(res, "_Z14k_track_klt_kfILi9E", facc)
    check_pair(new, old, BEFORE["k_track_klt<9>"][facc])
