"""k_remap (ov2slam_amd/csrc/rectify.hip): a device-only compile for gfx950 shows no scratch and at most 128 VGPRs, and the C ABI
of the rectification rejects bad arguments without a GPU (OV2_EINVAL before any device work: the map contract is checked on the
host, ahead of the context).  A map that does not match a tracker's or a pyramid's size needs both objects, hence a device: that
OV2_EINVAL is checked in tests/test_gpu_rectify.py."""
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
def test_k_remap_uses_no_scratch_and_at_most_128_vgprs(tmp_path):
    src = os.path.join(ROOT, "ov2slam_amd", "csrc", "rectify.hip")
    out = str(tmp_path / "rectify.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                    "--cuda-device-only", "-S", src, "-o", out], check=True, capture_output=True)
    txt = open(out).read()
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        res[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(private_segment_fixed_size|next_free_vgpr) (\d+)\s", m.group(2))}
    names = [n for n in res if "k_remap" in n]
    assert len(names) == 1, names
    r = res[names[0]]
    assert r["private_segment_fixed_size"] == 0, r
    assert r["next_free_vgpr"] <= 128, r


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _create(lib, ctx, w, h, form, m1, m2):
    out = C.c_void_p(0x1)
    rc = lib.ov2_rectmap_create(ctx, w, h, form, None if m1 is None else _p(m1), None if m2 is None else _p(m2), C.byref(out))
    assert out.value is None                        # *out is cleared on every failure
    return rc, lib.ov2_last_error()


def test_bad_arguments_are_einval_without_a_gpu():
    import ov2slam_amd
    from ov2slam_amd import _lib as L
    lib = ov2slam_amd.load()
    w, h = 8, 6
    mx = np.tile(np.arange(w, dtype=np.float32), (h, 1)); my = np.tile(np.arange(h, dtype=np.float32)[:, None], (1, w))
    fix1 = np.zeros((h, w, 2), np.int16); fix2 = np.zeros((h, w), np.uint16)
    # NULL out / maps / context
    assert lib.ov2_rectmap_create(None, w, h, L.OV2_MAP_F32, _p(mx), _p(my), None) == L.OV2_EINVAL
    rc, msg = _create(lib, None, w, h, L.OV2_MAP_F32, None, my)
    assert rc == L.OV2_EINVAL and b"NULL map" in msg
    rc, msg = _create(lib, None, w, h, L.OV2_MAP_F32, mx, my)           # a valid map: the NULL context is what is wrong
    assert rc == L.OV2_EINVAL and b"ctx == NULL" in msg
    rc, msg = _create(lib, None, w, h, L.OV2_MAP_FIXED, fix1, fix2)
    assert rc == L.OV2_EINVAL and b"ctx == NULL" in msg
    # form and size
    rc, msg = _create(lib, None, w, h, 2, mx, my)
    assert rc == L.OV2_EINVAL and b"form" in msg
    for bw, bh in ((1, h), (w, 1), (32768, h), (w, 32768), (0, 0), (-3, h)):
        rc, msg = _create(lib, None, bw, bh, L.OV2_MAP_F32, mx, my)
        assert rc == L.OV2_EINVAL and b"map size" in msg, (bw, bh)
    # OV2_MAP_F32: finite, |v| * 32 < 2^31
    for bad in (np.nan, np.inf, -np.inf):
        for which in (0, 1):
            m = [mx.copy(), my.copy()]
            m[which][h - 1, w - 1] = bad
            rc, msg = _create(lib, None, w, h, L.OV2_MAP_F32, m[0], m[1])
            assert rc == L.OV2_EINVAL and b"non-finite" in msg
    for bad in (2.0 ** 26, -2.0 ** 26, 3e9):
        m = mx.copy(); m[2, 3] = bad
        rc, msg = _create(lib, None, w, h, L.OV2_MAP_F32, m, my)
        assert rc == L.OV2_EINVAL and b"does not fit" in msg
    m = mx.copy(); m[2, 3] = np.float32(2.0 ** 26) * np.float32(1 - 2.0 ** -24)      # the largest float below 2^26 is inside the contract
    rc, msg = _create(lib, None, w, h, L.OV2_MAP_F32, m, my)
    assert rc == L.OV2_EINVAL and b"ctx == NULL" in msg
    # OV2_MAP_FIXED: map2 < 1024
    for bad in (1024, 65535):
        f2 = fix2.copy(); f2[h - 1, 0] = bad
        rc, msg = _create(lib, None, w, h, L.OV2_MAP_FIXED, fix1, f2)
        assert rc == L.OV2_EINVAL and b">= 1024" in msg
    f2 = fix2.copy(); f2[h - 1, 0] = 1023
    rc, msg = _create(lib, None, w, h, L.OV2_MAP_FIXED, fix1, f2)
    assert rc == L.OV2_EINVAL and b"ctx == NULL" in msg
    # the calls that take a map: NULL context / map / tracker / pyramid
    img = np.zeros((h, w), np.uint8)
    assert lib.ov2_rectify_h(None, None, _p(img), w, _p(img), w) == L.OV2_EINVAL and b"NULL" in lib.ov2_last_error()
    assert lib.ov2_rectify_d(None, None, None, w, 0, 1, None, w, 0) == L.OV2_EINVAL and b"NULL" in lib.ov2_last_error()
    assert lib.ov2_pyr_build_rect_h(None, None, None, 1, None, w, 1, 3.0, 1, 1) == L.OV2_EINVAL and b"NULL" in lib.ov2_last_error()
    assert lib.ov2_tracker_set_rectification(None, None) == L.OV2_EINVAL and b"NULL" in lib.ov2_last_error()
    assert lib.ov2_btracker_set_rectification(None, None) == L.OV2_EINVAL and b"NULL" in lib.ov2_last_error()
    lib.ov2_rectmap_destroy(None)                                        # a no-op
