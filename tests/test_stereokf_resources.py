"""Scope row f22 without a GPU: the new symbols are in the header, the built library and the bindings; the ABI version is still 600;
the header still compiles as C99 and the new ctypes structs lay out like it; every new entry point refuses a NULL tracker; the kernels
of csrc/stereokf.hip use no scratch and the registers and LDS DESIGN 4.26 states; and bt_skf_layout of csrc/trackb_layout.hpp is
checked with g++ as tests/test_lockstep_layout.py checks the others.  Only the code objects' metadata is read."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NEW = ("ov2_btracker_stereo_keyframe_begin", "ov2_btracker_stereo_keyframe_end", "ov2_btracker_stereo_keyframe",
       "ov2_btracker_get_keyframe_info")
# kernel -> (static LDS bytes, VGPR bound).  k_skf_input: the cell of each of OV2_FKF_MAX_POINTS keypoints (4 bytes); it runs the left
# camera's undistortion in fp64 next to the grid counts and stays under 96 VGPRs (five wavefronts per SIMD); k_skf_apply: six totals per
# wavefront; the two per-slot kernels: none, and eight wavefronts per SIMD stay possible
WANT = {"k_skf_input": (2048 * 4, 96), "k_skf_seed": (0, 64), "k_skf_stereo_kp": (0, 64), "k_skf_apply": (4 * 6 * 4, 64)}


def _section_426():
    txt = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"^#+ 4\.26 .*?(?=^#+ (?:4\.27|5)\b)", txt, re.S | re.M)
    assert m, "DESIGN.md has no section 4.26"
    return m.group(0)


def test_symbols_bindings_and_abi_version():
    import ov2slam_amd
    from ov2slam_amd import _lib as L
    from ov2slam_amd import mapper
    lib = ov2slam_amd.load()
    hdr = open(os.path.join(ROOT, "include", "ov2slam_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in L.SIGNATURES and name + "(" in hdr, name
    for name in ("stereoKeyframe", "stereoKeyframeBegin", "stereoKeyframeEnd", "getKeyframeInfo"):
        assert callable(getattr(ov2slam_amd.LockstepTracker, name)), name
    assert callable(mapper.stereo_keyframe_params)
    assert (L.OV2_SKF_NOT_REQUESTED, L.OV2_SKF_NOT_KEYFRAME, L.OV2_SKF_DONE) == (0, 1, 2)
    for words in ("#define OV2_SKF_NOT_REQUESTED 0", "#define OV2_SKF_NOT_KEYFRAME  1", "#define OV2_SKF_DONE          2"):
        assert words in hdr, words
    assert lib.ov2_version() == L.OV2_ABI_VERSION == 600 and "#define OV2_ABI_VERSION 600" in hdr
    # the header says what the call is and what it is not: the deviation, the absent state, the pass left out
    for words in ("(f22)", "k_skf_input", "k_skf_seed", "k_skf_stereo_kp", "k_skf_apply", "STAND IN SLOT ORDER", "CANNOT OCCUR",
                  "OUT OF SCOPE", "vgridkps_"):
        assert words in hdr, words
    mk = open(os.path.join(ROOT, "ov2slam_amd", "csrc", "Makefile")).read()
    assert "stereokf_dev.hpp" in mk
    # every field of the params struct names where it comes from
    body = re.search(r"typedef struct \{((?:(?!typedef).)*?)\} ov2_stereo_keyframe_params;", hdr, re.S).group(1)
    fields = [l for l in body.splitlines() if l.strip()]
    assert len(fields) == 17 and all("/*" in l and ("ov2_" in l) for l in fields), fields
    # the existing kernel files gained launchers, not kernels
    csrc = os.path.join(ROOT, "ov2slam_amd", "csrc")
    for f, n in (("priors.hip", 2), ("stereo.hip", 2), ("triangulate.hip", 1), ("stereokf.hip", 4)):
        assert open(os.path.join(csrc, f)).read().count("__global__") == n, f


def test_header_compiles_as_c99_and_the_new_structs_lay_out_like_it(tmp_path):
    from ov2slam_amd import _lib as L
    pairs = (("ov2_stereo_keyframe_params", L.StereoKeyframeParams), ("ov2_stereo_keyframe_result", L.StereoKeyframeResult))
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
    assert C.sizeof(L.StereoKeyframeResult) == 32                                   # BT_SKF_REC_BYTES
    # the same sizes from g++, which is what hipcc's host pass sees
    cpp = tmp_path / "sizes.cpp"
    cpp.write_text('#include <cstdio>\n#include "ov2slam_hip.h"\nint main() { printf("%zu %zu\\n", sizeof(ov2_stereo_keyframe_params), '
                   'sizeof(ov2_stereo_keyframe_result)); return 0; }\n')
    exe2 = tmp_path / "sizes"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(cpp), "-o", str(exe2)])
    sizes = [int(v) for v in subprocess.run([str(exe2)], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [C.sizeof(L.StereoKeyframeParams), C.sizeof(L.StereoKeyframeResult)]


def test_rejected_without_a_tracker():
    import ov2slam_amd
    from ov2slam_amd import _lib as L
    lib = ov2slam_amd.load()
    p = L.StereoKeyframeParams()
    do = (C.c_uint8 * 1)(1)
    R = (L.StereoKeyframeResult * 1)()
    C.memset(R, 0x6E, C.sizeof(R))
    i, t, n, hi = C.c_int(0x6E6E), C.c_double(6.5), C.c_int(0x6E6E), C.c_int(0x6E6E)
    assert lib.ov2_btracker_stereo_keyframe_begin(None, 1, C.byref(p), None, do) == L.OV2_EINVAL and b"NULL tracker" in lib.ov2_last_error()
    assert lib.ov2_btracker_stereo_keyframe_end(None, R, None, None, None, None, None) == L.OV2_EINVAL and b"NULL tracker" in lib.ov2_last_error()
    assert lib.ov2_btracker_stereo_keyframe(None, 1, C.byref(p), None, do, R, None, None, None, None, None) == L.OV2_EINVAL
    assert lib.ov2_btracker_get_keyframe_info(None, 0, 1, C.byref(i), C.byref(t), C.byref(n), C.byref(hi)) == L.OV2_EINVAL
    assert b"NULL tracker" in lib.ov2_last_error()
    assert (i.value, t.value, n.value, hi.value) == (0x6E6E, 6.5, 0x6E6E, 0x6E6E) and bytes(R) == b"\x6e" * C.sizeof(R)


def _resources(name):
    src = os.path.join(ROOT, "ov2slam_amd", "csrc", name + ".hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "--cuda-device-only",
                        "-S", src, "-o", "-"], check=True, capture_output=True, text=True)
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", r.stdout, re.S):
        res[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)\s", m.group(2))}
    return res


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_new_kernels_use_no_scratch_and_the_stated_registers_and_lds():
    res = _resources("stereokf")
    assert len(res) == 4, sorted(res)
    sec = _section_426()
    for k, (lds, vmax) in WANT.items():
        hits = [v for name, v in res.items() if k in name]
        assert len(hits) == 1, (k, sorted(res))
        r = hits[0]
        print(k, "vgpr", r["next_free_vgpr"], "sgpr", r["next_free_sgpr"], "lds", r["group_segment_fixed_size"])
        assert r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] == lds, (k, r)
        assert r["next_free_vgpr"] <= vmax, (k, r)
        # DESIGN 4.26 carries the figures of this build: "| k_skf_input | <vgpr> | <lds> |"
        row = re.search(r"\|\s*`?%s`?\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|" % k, sec)
        assert row, "DESIGN 4.26 has no resource row for " + k
        assert (int(row.group(1)), int(row.group(2))) == (r["next_free_vgpr"], lds), (k, row.group(0), r)


LAYOUT_SRC = r"""
#include <cstdio>
#include "trackb_layout.hpp"
int main()
{
    printf("const %d\n", BT_SKF_REC_BYTES);
    const int cases[][3] = {{1, 1, 0}, {4, 160, 77}, {2, 160, 20}, {11, 308, 308}, {4096, 308, 0}, {4096, 308, 308}, {64, 2048, 65536}};
    for (auto &c : cases) {
        const BtSkfLayout L = bt_skf_layout(c[0], c[1], c[2]);
        const size_t v[] = {L.s_act, L.s_up, L.s_io, L.s_rec, L.s_rpx, L.s_wpt, L.s_inv, L.s_sok, L.s_tst, L.s_down, L.w_pit, L.w_tit, L.w_Tcw,
                            L.w_Twc, L.w_nd, L.w_px, L.w_un, L.w_bv, L.w_fw, L.w_top, L.w_pri, L.w_out, L.w_gru, L.w_ru, L.w_rbv, L.w_src,
                            L.w_sx, L.w_l1, L.w_err, L.w_st, L.w_hp, L.w_sk, L.w_fl, L.w_lk, L.w_ok, L.w_is, L.w_cs, L.w_ck, L.dev_bytes};
        printf("%d %d %d", c[0], c[1], c[2]);
        for (size_t x : v) printf(" %zu", x);
        printf("\n");
    }
    return 0;
}
"""


def test_skf_layout(tmp_path):
    """bt_skf_layout against the restatement below: [act 1 per item] goes up; [record 32 per item][right_px 8][wpt 24][invdepth 8]
    [stereo_ok 1][tri_status 1 per slot] come down; behind them the device-only ranges per item (16, 16, 56, 56, 4 bytes), per slot
    (8 8 24 24 8 8 8 8 8 24 4 4 4 4 and seven of 1) and the grid (4 per cell + 1 per item, 4 per slot); 256-byte starts, no section
    reaching into the next; nothing in front of the grid depends on the cells"""
    cpp, exe = tmp_path / "t.cpp", tmp_path / "t"
    cpp.write_text(LAYOUT_SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "ov2slam_amd", "csrc"), str(cpp), "-o", str(exe)])
    lines = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    assert lines[0].split() == ["const", "32"]
    assert len(lines) == 8
    up256 = lambda v: (v + 255) & ~255
    seen = {}
    for line in lines[1:]:
        v = [int(x) for x in line.split()]
        B, nm, cells, got = v[0], v[1], v[2], v[3:]
        slots, o, want = B * nm, 0, []

        def take(n):
            nonlocal o
            want.append(o)
            o = up256(o + n)
        take(B)
        want.append(o)                                                   # s_up
        want.append(o)                                                   # s_io = s_rec
        for n in (32 * B, 8 * slots, 24 * slots, 8 * slots, slots, slots):
            take(n)
        want.append(o)                                                   # s_down
        for n in (16 * B, 16 * B, 56 * B, 56 * B, 4 * B):
            take(n)
        for per in (8, 8, 24, 24, 8, 8, 8, 8, 8, 24, 4, 4, 4, 4, 1, 1, 1, 1, 1, 1, 1):
            take(per * slots)
        take(4 * (cells + 1) * B)
        take(4 * slots)
        want.append(o)                                                   # dev_bytes
        assert got == want, (B, nm, cells, got, want)
        assert all(x % 256 == 0 for x in want)
        front = seen.setdefault((B, nm), got[:-2])                       # everything up to and including w_cs
        assert front == got[:-2]
