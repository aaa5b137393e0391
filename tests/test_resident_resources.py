"""Scope row f21 without a GPU: the new symbols are in the header, the built library and the bindings; the ABI version is still 600;
the header still compiles as C99 and the new ctypes structs lay out like it; every new entry point refuses a NULL tracker; the kernels
of csrc/resident.hip use no scratch, at most 64 VGPRs and the LDS DESIGN 4.25 states; and bt_res_layout of csrc/trackb_layout.hpp is
checked with g++ as tests/test_lockstep_layout.py checks the others.  Only the code objects' metadata is read."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NEW = ("ov2_btracker_set_frame", "ov2_btracker_get_frame", "ov2_btracker_update_frame", "ov2_btracker_update_frame_batch",
       "ov2_btracker_track_mono_resident_begin", "ov2_btracker_track_mono_resident_end", "ov2_btracker_track_mono_resident",
       "ov2_btracker_last_slot_bytes")


def test_symbols_bindings_and_abi_version():
    import ov2slam_amd
    from ov2slam_amd import _lib as L
    lib = ov2slam_amd.load()
    hdr = open(os.path.join(ROOT, "include", "ov2slam_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in L.SIGNATURES and name + "(" in hdr, name
    for name in ("setFrame", "getFrame", "updateFrame", "trackMonoResident", "trackMonoResidentBegin", "trackMonoResidentEnd", "lastSlotBytes",
                 "createKeyframe"):
        assert callable(getattr(ov2slam_amd.LockstepTracker, name)), name
    assert (L.OV2_RES_SET_POINT, L.OV2_RES_UNSET_POINT, L.OV2_RES_REMOVE) == (0, 1, 2)
    for words in ("#define OV2_RES_SET_POINT   0", "#define OV2_RES_UNSET_POINT 1", "#define OV2_RES_REMOVE      2"):
        assert words in hdr, words
    assert lib.ov2_version() == L.OV2_ABI_VERSION == 600 and "#define OV2_ABI_VERSION 600" in hdr
    for words in ("(f21)", "k_res_update", "k_res_stage", "k_res_carry", "k_res_ckf_in", "k_res_adopt", "input->px_h == NULL",
                  "lmid repeated within one item's list"):
        assert words in hdr, words
    mk = open(os.path.join(ROOT, "ov2slam_amd", "csrc", "Makefile")).read()
    assert "resident_dev.hpp" in mk
    # k_mono_pack's rule is restated in the new header, not edited in place, and stands there once
    dev = open(os.path.join(ROOT, "ov2slam_amd", "csrc", "resident_dev.hpp")).read()
    assert dev.count("bool res_keep(") == 1 and "(status[s] & 3) == 1" in dev


def test_header_compiles_as_c99_and_the_new_structs_lay_out_like_it(tmp_path):
    from ov2slam_amd import _lib as L
    pairs = (("ov2_resident_op", L.ResidentOp), ("ov2_resident_update_result", L.ResidentUpdateResult),
             ("ov2_resident_step_result", L.ResidentStepResult))
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
    assert (C.sizeof(L.ResidentOp), C.sizeof(L.ResidentUpdateResult), C.sizeof(L.ResidentStepResult)) == (32, 24, 8)      # BT_RES_OP_BYTES, BT_RES_REC_BYTES


def test_rejected_without_a_tracker():
    import ov2slam_amd
    from ov2slam_amd import _lib as L
    lib = ov2slam_amd.load()
    n, nops = C.c_int(0x6E6E), C.c_int(0)
    op = (L.ResidentOp * 1)()
    ops = (C.POINTER(L.ResidentOp) * 1)(C.cast(op, C.POINTER(L.ResidentOp)))
    R = (L.ResidentUpdateResult * 1)()
    F = (L.ResidentStepResult * 1)()
    P, M = (L.PoseResult * 1)(), (L.TrackMonoResult * 1)()
    mp, mi = L.TrackMonoParams(), L.TrackMonoInput()
    v = C.c_size_t(77)
    for buf in (R, F, M):
        C.memset(buf, 0x6E, C.sizeof(buf))
    assert lib.ov2_btracker_set_frame(None, 0, 0, None, None, None, None) == L.OV2_EINVAL and b"NULL tracker" in lib.ov2_last_error()
    assert lib.ov2_btracker_get_frame(None, 0, 1, C.byref(n), None, None, None, None) == L.OV2_EINVAL and b"NULL tracker" in lib.ov2_last_error()
    assert lib.ov2_btracker_update_frame(None, 0, 0, op, R) == L.OV2_EINVAL
    assert lib.ov2_btracker_update_frame_batch(None, 1, C.byref(nops), ops, R) == L.OV2_EINVAL
    assert lib.ov2_btracker_track_mono_resident_begin(None, 1, None, 0, 1, C.byref(mp), C.byref(mi)) == L.OV2_EINVAL
    assert lib.ov2_btracker_track_mono_resident_end(None, None, None, None, None, P, M, F) == L.OV2_EINVAL and b"NULL tracker" in lib.ov2_last_error()
    assert lib.ov2_btracker_track_mono_resident(None, 1, None, 0, 1, C.byref(mp), C.byref(mi), None, None, None, None, P, M, F) == L.OV2_EINVAL
    assert lib.ov2_btracker_last_slot_bytes(None, C.byref(v)) == L.OV2_EINVAL
    assert n.value == 0x6E6E and v.value == 77 and all(bytes(buf) == b"\x6e" * C.sizeof(buf) for buf in (R, F, M))


def _resources(name):
    src = os.path.join(ROOT, "ov2slam_amd", "csrc", name + ".hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "--cuda-device-only",
                        "-S", src, "-o", "-"], check=True, capture_output=True, text=True)
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", r.stdout, re.S):
        res[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)\s", m.group(2))}
    return res


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_new_kernels_use_no_scratch_and_at_most_64_vgprs():
    res = _resources("resident")
    assert len(res) == 5, sorted(res)
    # static LDS.  k_res_update: OV2_FKF_MAX_POINTS op ids (4 bytes) and op codes (1 byte), two sets of four wavefront counts and three
    # totals per wavefront; k_res_carry: the two sets of counts; the others: none
    want = {"k_res_update": 2048 * 4 + 2048 + 32 + 48, "k_res_stage": 0, "k_res_carry": 32, "k_res_ckf_in": 0, "k_res_adopt": 0}
    for k, lds in want.items():
        hits = [v for name, v in res.items() if k in name]
        assert len(hits) == 1, (k, sorted(res))
        r = hits[0]
        print(k, "vgpr", r["next_free_vgpr"], "sgpr", r["next_free_sgpr"], "lds", r["group_segment_fixed_size"])
        assert r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] == lds, (k, r)
        assert r["next_free_vgpr"] <= 64, (k, r)                     # eight wavefronts per SIMD stay possible


LAYOUT_SRC = r"""
#include <cstdio>
#include "trackb_layout.hpp"
int main()
{
    printf("const %d %d\n", BT_RES_OP_BYTES, BT_RES_REC_BYTES);
    const int cases[][2] = {{1, 1}, {4, 160}, {11, 308}, {4096, 308}, {65535, 2048}};
    for (auto &c : cases) {
        const BtResLayout L = bt_res_layout(c[0], c[1]);
        printf("%d %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", c[0], c[1], L.f_n, L.f_px, L.f_lm, L.f_3d, L.f_w, L.f_item,
               L.buf_bytes, L.frame_bytes, L.u_sel, L.u_nop, L.u_off, L.u_ops, L.u_up, L.u_rec, L.ctl_bytes);
    }
    return 0;
}
"""


def test_res_layout(tmp_path):
    """bt_res_layout against the restatement below.  The frame block: an item is [n][px 8][lmid 4][is3d 1][wpt 24 per slot] with
    16-byte starts in a multiple of 256 bytes, a buffer is `batch` items, the block two buffers.  The control block: [sel 1][n_ops 4]
    [first op 4 per item][ops 32 per slot] go up, [record 24 per item] comes down, 256-byte starts, no section reaching into the next"""
    cpp, exe = tmp_path / "t.cpp", tmp_path / "t"
    cpp.write_text(LAYOUT_SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "ov2slam_amd", "csrc"), str(cpp), "-o", str(exe)])
    lines = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    assert lines[0].split() == ["const", "32", "24"]
    assert len(lines) == 6
    up16, up256 = (lambda v: (v + 15) & ~15), (lambda v: (v + 255) & ~255)
    for line in lines[1:]:
        v = [int(x) for x in line.split()]
        B, nm, got = v[0], v[1], v[2:]
        offs, o = [], 0
        for n in (4, 8 * nm, 4 * nm, nm, 24 * nm):
            offs.append(o)
            o = up16(o + n)
        item = up256(o)
        want = offs + [item, item * B, 2 * item * B]
        slots, o = B * nm, 0
        for n in (B, 4 * B, 4 * B, 32 * slots):
            want.append(o)
            o = up256(o + n)
        want += [o, o, up256(o + 24 * B)]                                # u_up, u_rec, ctl_bytes
        assert got == want, (B, nm, got, want)
        assert all(x % 16 == 0 for x in want[:5]) and all(x % 256 == 0 for x in want[5:])
