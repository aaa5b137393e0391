"""k_fb_klt3 (ov2slam_amd/csrc/lk3.hip) runs four wavefronts per SIMD: at most 128 VGPRs, no scratch, and at most
10 240 B of LDS per work-group (16 single-wavefront work-groups per CU).  A device-only compile for gfx950 checks the
three limits, so that a change to the kernel cannot lose the occupancy silently.  No GPU needed; skipped without hipcc."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def kernel_resources(tmp_path, *flags):
    """{kernel name: {field: int}} from the .amdhsa_kernel blocks of lk3.hip's device assembly."""
    src = os.path.join(ROOT, "ov2slam_amd", "csrc", "lk3.hip")
    out = str(tmp_path / "lk3.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                    "--cuda-device-only", "-S", *flags, src, "-o", out], check=True, capture_output=True)
    txt = open(out).read()
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        res[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)\s", m.group(2))}
    return res


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_k_fb_klt3_fits_four_waves_per_simd(tmp_path):
    res = kernel_resources(tmp_path)
    names = [n for n in res if "k_fb_klt3" in n]
    assert len(names) == 1, names
    r = res[names[0]]
    assert r["next_free_vgpr"] <= 128, r["next_free_vgpr"]                 # 512 / 128 = 4 wavefronts per SIMD
    assert r["accum_offset"] <= 128, r["accum_offset"]
    assert r["private_segment_fixed_size"] == 0, r["private_segment_fixed_size"]   # no spills
    assert r["group_segment_fixed_size"] <= 10240, r["group_segment_fixed_size"]   # 16 work-groups in 160 KB of LDS
