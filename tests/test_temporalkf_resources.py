"""Scope row f23 without a GPU: the new symbols are in the header, the built library and the bindings; the ABI version is still 600;
the header still compiles as C99 and the new ctypes structs lay out like it; every new entry point refuses a NULL tracker; the kernels
of csrc/temporalkf.hip use no scratch and the registers and LDS DESIGN 4.27 states; and bt_tkf_layout of csrc/trackb_layout.hpp is
checked with g++ as tests/test_lockstep_layout.py checks the others.  Only the code objects' metadata is read."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NEW = ("ov2_btracker_temporal_keyframe_begin", "ov2_btracker_temporal_keyframe_end", "ov2_btracker_temporal_keyframe",
       "ov2_btracker_reserve_anchors", "ov2_btracker_set_anchors", "ov2_btracker_get_anchors", "ov2_btracker_set_anchor_poses_batch",
       "ov2_btracker_set_anchor_poses")
# kernel -> (static LDS bytes, VGPR bound).  k_tkf_anchor: one mark per row of OV2_TKF_MAX_ROWS (4 bytes); k_tkf_apply: one byte per
# keypoint of OV2_FKF_MAX_POINTS, five totals per wavefront and res_rank's two sets of four counts; the per-slot and per-triple
# kernels: none.  All of them stay at 64 VGPRs or fewer: eight wavefronts per SIMD stay possible.
WANT = {"k_tkf_anchor": (256 * 4, 64), "k_tkf_input": (0, 64), "k_tkf_apply": (2048 + 4 * 5 * 4 + 2 * 4 * 4, 64), "k_tkf_set_poses": (0, 64)}


def _section_427():
    txt = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"^#+ 4\.27 .*?(?=^#+ (?:4\.28|5)\b)", txt, re.S | re.M)
    assert m, "DESIGN.md has no section 4.27"
    return m.group(0)


def test_symbols_bindings_and_abi_version():
    import ov2slam_amd
    from ov2slam_amd import _lib as L
    from ov2slam_amd import mapper
    lib = ov2slam_amd.load()
    hdr = open(os.path.join(ROOT, "include", "ov2slam_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in L.SIGNATURES and name + "(" in hdr, name
    for name in ("temporalKeyframe", "temporalKeyframeBegin", "temporalKeyframeEnd", "setAnchors", "getAnchors", "setAnchorPoses", "reserveAnchors"):
        assert callable(getattr(ov2slam_amd.LockstepTracker, name)), name
    assert callable(mapper.temporal_keyframe_params)
    p = mapper.temporal_keyframe_params(dict(K=(1, 2, 3, 4), iK=range(9), Kr=(1, 2, 3, 4), Tlr=range(7), Tcic0=range(7), stereo=True, rect=False,
                                             fmax_reproj_err=3.0), n_src_max=8)
    assert p.n_src_max == 8 and p.tri.stereo == 1 and list(p.tri.K) == [1, 2, 3, 4]
    assert (L.OV2_TKF_NOT_REQUESTED, L.OV2_TKF_NOT_KEYFRAME, L.OV2_TKF_DONE, L.OV2_TKF_SRC_OVERFLOW, L.OV2_TKF_MAX_ROWS) == (0, 1, 2, 3, 256)
    for words in ("#define OV2_TKF_NOT_REQUESTED 0", "#define OV2_TKF_NOT_KEYFRAME  1", "#define OV2_TKF_DONE          2",
                  "#define OV2_TKF_SRC_OVERFLOW  3", "#define OV2_TKF_MAX_ROWS      256"):
        assert words in hdr, words
    assert lib.ov2_version() == L.OV2_ABI_VERSION == 600 and "#define OV2_ABI_VERSION 600" in hdr
    # the header says what the call is and what it is not: the anchor table, the absent cases, the deviation
    for words in ("(f23)", "k_tkf_anchor", "k_tkf_input", "k_tkf_apply", "k_tkf_set_poses", "THE ANCHOR TABLE", "CANNOT OCCUR", "ONE DEVIATION",
                  "plm == nullptr", "pkf == nullptr", "removeMapPointObs"):
        assert words in hdr, words
    mk = open(os.path.join(ROOT, "ov2slam_amd", "csrc", "Makefile")).read()
    assert "temporalkf_dev.hpp" in mk
    # no existing kernel file gained or lost a kernel; the new file holds four
    csrc = os.path.join(ROOT, "ov2slam_amd", "csrc")
    for f, n in (("triangulate.hip", 1), ("stereokf.hip", 4), ("createkf.hip", 3), ("temporalkf.hip", 4)):
        assert open(os.path.join(csrc, f)).read().count("__global__") == n, f


def test_header_compiles_as_c99_and_the_new_structs_lay_out_like_it(tmp_path):
    from ov2slam_amd import _lib as L
    pairs = (("ov2_temporal_keyframe_params", L.TemporalKeyframeParams), ("ov2_temporal_keyframe_result", L.TemporalKeyframeResult))
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
    assert C.sizeof(L.TemporalKeyframeResult) == 32                                 # BT_TKF_REC_BYTES
    # the same sizes from g++, which is what hipcc's host pass sees
    cpp = tmp_path / "sizes.cpp"
    cpp.write_text('#include <cstdio>\n#include "ov2slam_hip.h"\nint main() { printf("%zu %zu\\n", sizeof(ov2_temporal_keyframe_params), '
                   'sizeof(ov2_temporal_keyframe_result)); return 0; }\n')
    exe2 = tmp_path / "sizes"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(cpp), "-o", str(exe2)])
    sizes = [int(v) for v in subprocess.run([str(exe2)], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [C.sizeof(L.TemporalKeyframeParams), C.sizeof(L.TemporalKeyframeResult)]


def test_rejected_without_a_tracker():
    import ov2slam_amd
    from ov2slam_amd import _lib as L
    lib = ov2slam_amd.load()
    p = L.TemporalKeyframeParams()
    p.n_src_max = 8
    do = (C.c_uint8 * 1)(1)
    R = (L.TemporalKeyframeResult * 1)()
    C.memset(R, 0x6E, C.sizeof(R))
    n, nr, ign = C.c_int(0x6E6E), C.c_int(0x6E6E), C.c_int(0x6E6E)
    one, T = (C.c_int * 1)(0), (C.c_double * 7)(0, 0, 0, 0, 0, 0, 1)
    assert lib.ov2_btracker_temporal_keyframe_begin(None, 1, C.byref(p), do) == L.OV2_EINVAL and b"NULL tracker" in lib.ov2_last_error()
    assert lib.ov2_btracker_temporal_keyframe_end(None, R, None, None, None, None) == L.OV2_EINVAL and b"NULL tracker" in lib.ov2_last_error()
    assert lib.ov2_btracker_temporal_keyframe(None, 1, C.byref(p), do, R, None, None, None, None) == L.OV2_EINVAL
    assert lib.ov2_btracker_reserve_anchors(None, 8) == L.OV2_EINVAL and b"NULL tracker" in lib.ov2_last_error()
    assert lib.ov2_btracker_set_anchors(None, 0, 0, None, None, None, None, 0, None, None) == L.OV2_EINVAL and b"NULL tracker" in lib.ov2_last_error()
    assert lib.ov2_btracker_get_anchors(None, 0, 1, C.byref(n), None, None, None, None, C.byref(nr), None, None, None) == L.OV2_EINVAL
    assert b"NULL tracker" in lib.ov2_last_error()
    assert lib.ov2_btracker_set_anchor_poses_batch(None, 1, one, one, T, C.byref(ign)) == L.OV2_EINVAL and b"NULL tracker" in lib.ov2_last_error()
    assert lib.ov2_btracker_set_anchor_poses(None, 0, 1, one, T, C.byref(ign)) == L.OV2_EINVAL and b"NULL tracker" in lib.ov2_last_error()
    assert (n.value, nr.value, ign.value) == (0x6E6E,) * 3 and bytes(R) == b"\x6e" * C.sizeof(R)


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
    res = _resources("temporalkf")
    assert len(res) == 4, sorted(res)
    sec = _section_427()
    for k, (lds, vmax) in WANT.items():
        hits = [v for name, v in res.items() if k in name]
        assert len(hits) == 1, (k, sorted(res))
        r = hits[0]
        print(k, "vgpr", r["next_free_vgpr"], "sgpr", r["next_free_sgpr"], "lds", r["group_segment_fixed_size"])
        assert r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] == lds, (k, r)
        assert r["next_free_vgpr"] <= vmax, (k, r)
        # DESIGN 4.27 carries the figures of this build: "| k_tkf_anchor | <vgpr> | <lds> |"
        row = re.search(r"\|\s*`?%s`?\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|" % k, sec)
        assert row, "DESIGN 4.27 has no resource row for " + k
        assert (int(row.group(1)), int(row.group(2))) == (r["next_free_vgpr"], lds), (k, row.group(0), r)


LAYOUT_SRC = r"""
#include <cstdio>
#include "trackb_layout.hpp"
int main()
{
    printf("const %d\n", BT_TKF_REC_BYTES);
    const int cases[][3] = {{1, 1, 1}, {4, 160, 8}, {4, 160, 2}, {11, 308, 16}, {4096, 308, 8}, {64, 2048, 256}};
    for (auto &c : cases) {
        const BtTkfLayout L = bt_tkf_layout(c[0], c[1], c[2]);
        const size_t v[] = {L.a_n, L.a_lm, L.a_row, L.a_un, L.a_bv, L.a_nr, L.a_kf, L.a_Twc, L.a_Tcw, L.a_item, L.buf_bytes, L.anchor_bytes,
                            L.t_act, L.t_sel, L.t_up, L.t_io, L.t_rec, L.t_wpt, L.t_inv, L.t_skf, L.t_tst, L.t_down,
                            L.w_tit, L.w_Twc, L.w_ovf, L.w_srcT, L.w_un, L.w_bv, L.w_sun, L.w_sbv, L.w_src, L.w_is, L.dev_bytes,
                            L.p_item, L.p_kfid, L.p_Twc, L.pose_bytes};
        printf("%d %d %d", c[0], c[1], c[2]);
        for (size_t x : v) printf(" %zu", x);
        printf("\n");
    }
    return 0;
}
"""


def test_tkf_layout(tmp_path):
    """bt_tkf_layout against the restatement below.  One item of the anchor table: [n 4][lmid 4][row 4][unpx 8][bv 24 per slot][n_rows 4]
    [kfid 4][Twc 56][Tcw 56 per row], 16-byte starts, the item a multiple of 256, two buffers of `batch` items.  The call's block: [act 1]
    [asel 1 per item] go up; [record 32 per item][wpt 24][invdepth 8][src_kfid 4][tri_status 1 per slot] come down; behind them the
    device-only ranges per item (16, 56, 4 bytes), per row (112) and per slot (8 24 8 24 4 1); 256-byte starts, no section reaching
    into the next.  The pose block: [item 4][kfid 4][Twc 56] per row of the batch."""
    cpp, exe = tmp_path / "t.cpp", tmp_path / "t"
    cpp.write_text(LAYOUT_SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "ov2slam_amd", "csrc"), str(cpp), "-o", str(exe)])
    lines = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    assert lines[0].split() == ["const", "32"]
    assert len(lines) == 7
    for line in lines[1:]:
        v = [int(x) for x in line.split()]
        B, nm, ns, got = v[0], v[1], v[2], v[3:]
        slots, rows, want = B * nm, B * ns, []
        o = 0

        def take(n, align):
            nonlocal o
            want.append(o)
            o = (o + n + align - 1) & ~(align - 1)
        for n in (4, 4 * nm, 4 * nm, 8 * nm, 24 * nm, 4, 4 * ns, 56 * ns, 56 * ns):
            take(n, 16)
        item = (o + 255) & ~255
        want += [item, item * B, 2 * item * B]
        assert all(x % 8 == 0 for x in want[:9])                          # doubles and float2 on their alignment
        o = 0
        take(B, 256); take(B, 256)
        want.append(o)                                                   # t_up
        want.append(o)                                                   # t_io = t_rec
        for n in (32 * B, 24 * slots, 8 * slots, 4 * slots, slots):
            take(n, 256)
        want.append(o)                                                   # t_down
        for n in (16 * B, 56 * B, 4 * B, 112 * rows, 8 * slots, 24 * slots, 8 * slots, 24 * slots, 4 * slots, slots):
            take(n, 256)
        want.append(o)                                                   # dev_bytes
        assert all(x % 256 == 0 for x in want[12:])
        o = 0
        for n in (4 * rows, 4 * rows, 56 * rows):
            take(n, 256)
        want.append(o)                                                   # pose_bytes
        assert got == want, (B, nm, ns, got, want)
