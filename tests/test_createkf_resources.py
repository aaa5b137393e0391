"""Scope row f20 without a GPU: the new symbols are in the header, the built library and the bindings; the ABI version is still 600;
the header still compiles as C and the new ctypes structs lay out like it; the calls refuse a NULL tracker; the kernels of
csrc/createkf.hip use no scratch and at most 64 VGPRs, as their siblings k_epif_pack / k_mono_pack are held to; the kernels of the files
this row touches or calls into (detect.hip gained a per-item skip byte; brief.hip, keypoint.hip and mono.hip are only called) report the
resources of the commit before this one; and the new layout function of csrc/trackb_layout.hpp is checked with g++ as
tests/test_lockstep_layout.py checks the others.  Only the code objects' metadata is read."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NEW = ("ov2_btracker_create_keyframe_begin", "ov2_btracker_create_keyframe_end", "ov2_btracker_create_keyframe")


def _resources(name):
    src = os.path.join(ROOT, "ov2slam_amd", "csrc", name + ".hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "--cuda-device-only",
                        "-S", src, "-o", "-"], check=True, capture_output=True, text=True)
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", r.stdout, re.S):
        res[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)\s", m.group(2))}
    return res


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
    for name in ("createKeyframe", "createKeyframeBegin", "createKeyframeEnd"):
        assert callable(getattr(ov2slam_amd.LockstepTracker, name)), name
    assert (L.OV2_CKF_NOT_REQUESTED, L.OV2_CKF_CREATED, L.OV2_CKF_OVERFLOW, L.OV2_CKF_DUP_LMID) == (0, 1, 2, 3)
    assert "OV2_CKF_NOT_REQUESTED = 0, OV2_CKF_CREATED = 1, OV2_CKF_OVERFLOW = 2, OV2_CKF_DUP_LMID = 3" in hdr
    assert (L.OV2_CKF_DET_SINGLESCALE, L.OV2_CKF_DET_GRID_FAST, L.OV2_CKF_DET_GFTT) == (0, 1, 2)
    assert lib.ov2_version() == L.OV2_ABI_VERSION == 600 and "#define OV2_ABI_VERSION 600" in hdr
    for words in ("(f20;", "prepareFrame's filter", "so it stays with the caller", "k_ckf_prepare", "k_ckf_append", "k_ckf_install",
                  "Twc_h == NULL on a tracker without a resident pose", "detectGFTT is not fused"):
        assert words in hdr, words
    mk = open(os.path.join(ROOT, "ov2slam_amd", "csrc", "Makefile")).read()
    assert "detect_dev.hpp" in mk and "createkf_dev.hpp" in mk
    det = open(os.path.join(ROOT, "ov2slam_amd", "csrc", "detect.hip")).read()
    assert '#include "detect_dev.hpp"' in det and "struct DetBatch" not in det and "static int enqueue_detect" not in det        # one copy, exported


def test_header_compiles_as_c_and_the_new_structs_lay_out_like_it(tmp_path):
    from ov2slam_amd import _lib as L
    pairs = (("ov2_create_keyframe_params", L.CreateKeyframeParams), ("ov2_create_keyframe_input", L.CreateKeyframeInput),
             ("ov2_create_keyframe_result", L.CreateKeyframeResult))
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
    assert C.sizeof(L.CreateKeyframeResult) == 32                    # BT_CKF_REC_BYTES


def test_rejected_without_a_tracker():
    import ov2slam_amd
    from ov2slam_amd import _lib as L
    lib = ov2slam_amd.load()
    cp, ci = L.CreateKeyframeParams(), L.CreateKeyframeInput()
    R = (L.CreateKeyframeResult * 1)()
    C.memset(R, 0x6E, C.sizeof(R))
    assert lib.ov2_btracker_create_keyframe_begin(None, 1, C.byref(cp), C.byref(ci)) == L.OV2_EINVAL
    assert b"NULL tracker" in lib.ov2_last_error()
    assert lib.ov2_btracker_create_keyframe_end(None, R, None, None, None, None, None, None, None) == L.OV2_EINVAL
    assert lib.ov2_btracker_create_keyframe(None, 1, C.byref(cp), C.byref(ci), R, None, None, None, None, None, None, None) == L.OV2_EINVAL
    assert bytes(R) == b"\x6e" * C.sizeof(R)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_new_kernels_use_no_scratch_and_at_most_64_vgprs():
    res = _resources("createkf")
    assert len(res) == 3, sorted(res)
    # static LDS: the bitmap of OV2_FKF_MAX_CELLS cells and two counts; none; OV2_FKF_MAX_POINTS 8-byte sort keys and the flag
    for k, lds in (("k_ckf_prepare", 65536 // 8 + 8), ("k_ckf_append", 0), ("k_ckf_install", 2048 * 8 + 8)):
        r = _of(res, k)
        print(k, "vgpr", r["next_free_vgpr"], "sgpr", r["next_free_sgpr"], "lds", r["group_segment_fixed_size"])
        assert r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] == lds, (k, r)
        assert r["next_free_vgpr"] <= 64, (k, r)                     # eight wavefronts per SIMD stay possible


# (VGPRs, LDS bytes, scratch bytes) of the commit before this one, from a device-only compile of that commit's own tree.  The three
# wide k_grid_select instances of the single-scale mode carried their 8 bytes of scratch there already.
_SEL = "k_grid_selectILi%dELi%dELi%dELi%dEE"
PARENT = {"detect": dict([("k_fast_cells", (40, 8232, 0)), ("k_mineig_cells", (58, 256, 0)), ("k_free_cells", (17, 0, 0)),
                          ("k_mineig_strip", (64, 432, 0)), ("k_corner_subpixILi1EE", (60, 472, 0)), ("k_corner_subpixILi2EE", (62, 1208, 0)),
                          ("k_corner_subpixILi3EE", (66, 2296, 0)), ("k_corner_subpixILi4EE", (60, 3736, 0)),
                          ("k_corner_subpixILi5EE", (66, 5528, 0))]
                         + [(_SEL % (0, mr, ch, nt), (128, 80, 0)) for mr, ch in ((36, 1), (52, 1), (32, 2)) for nt in (1024, 512)]
                         + [(_SEL % (1, 36, 1, nt), (106, 80, 0)) for nt in (1024, 512)]
                         + [(_SEL % (1, mr, ch, nt), (128, 80, 8)) for mr, ch in ((52, 1), (32, 2)) for nt in (1024, 512)]),
          "brief": {"k_brief32": (73, 26912, 0)},
          "keypoint": {"k_compute_keypoints": (34, 0, 0)},
          "mono": {"k_mono_apply": (112, 0, 0), "k_mono_pack": (74, 32, 0)}}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("name", sorted(PARENT))
def test_surrounding_kernels_keep_their_resources(name):
    res = _resources(name)
    assert len(res) == len(PARENT[name]), sorted(res)
    for k, want in PARENT[name].items():
        r = _of(res, k)
        assert (r["next_free_vgpr"], r["group_segment_fixed_size"], r["private_segment_fixed_size"]) == want, (k, r)


LAYOUT_SRC = r"""
#include <cstdio>
#include "trackb_layout.hpp"
int main()
{
    printf("const %d %d %d\n", BT_CKF_REC_BYTES, BT_CKF_SO_BYTES, BT_KF_HDR_BYTES);
    const int cases[][2] = {{1, 1}, {4, 160}, {11, 308}, {4096, 308}, {65535, 2048}};
    for (auto &c : cases) {
        const BtCkfLayout L = bt_ckf_layout(c[0], c[1]);
        printf("%d %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", c[0], c[1], L.c_n,
               L.c_fl, L.c_nl, L.c_id, L.c_tm, L.c_T, L.c_par, L.c_3d, L.c_io, L.c_px, L.c_lm, L.c_up, L.c_rec, L.c_so, L.c_hdr, L.c_un, L.c_bv,
               L.c_col, L.c_perm, L.c_desc, L.c_val, L.c_down, L.w_skip, L.w_nb, L.dev_bytes);
    }
    return 0;
}
"""


def test_ckf_layout(tmp_path):
    """bt_ckf_layout against the restatement below: the documented order and sizes, 256-byte starts, no section reaching into the next,
    the upload prefix ending where the download-only part begins, the frame's px / lmid inside both, the descriptors last of what comes
    down, the device-only counts behind everything the host block holds"""
    cpp, exe = tmp_path / "t.cpp", tmp_path / "t"
    cpp.write_text(LAYOUT_SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "ov2slam_amd", "csrc"), str(cpp), "-o", str(exe)])
    lines = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    assert lines[0].split() == ["const", "32", "56", "120"]
    up = lambda v: (v + 255) & ~255
    assert len(lines) == 6
    for line in lines[1:]:
        v = [int(x) for x in line.split()]
        B, nm, got = v[0], v[1], v[2:]
        slots = B * nm
        sizes = [4 * B, B, 4 * B, 4 * B, 8 * B, 56 * B, 8 * B, slots,                    # up only
                 8 * slots, 4 * slots,                                                   # up and down
                 32 * B, 56 * B, 120 * B, 8 * slots, 24 * slots, slots, 4 * slots, 32 * slots, slots,      # down only
                 B, 4 * B]                                                               # device only
        offs, o = [], 0
        for n in sizes:
            offs.append(o)
            o = up(o + n)
        c_io, c_up, c_down = offs[8], offs[10], offs[19]
        want = offs[:8] + [c_io] + offs[8:10] + [c_up] + offs[10:19] + [c_down] + offs[19:] + [o]
        assert got == want, (B, nm, got, want)
        assert all(x % 256 == 0 for x in want)
