"""Scope row f19 without a GPU: the new symbols are in the header, the built library and the bindings; the ABI version is still 600;
the header still compiles as C and the new ctypes structs lay out like it; the calls refuse a NULL tracker and check their inputs
before they look at the context; the kernels of csrc/motion.hip and csrc/mono.hip use no scratch; the kernels whose SE(3) arithmetic
moved into csrc/se3_dev.hpp (posegraph.hip), whose inverse moved into a shared inline (frameepi.hip) and the decision kernel, now
reached through a launcher too (fkf.hip), report the resources of the commit before this one; and the new layout function of
csrc/trackb_layout.hpp is checked with g++ as tests/test_lockstep_layout.py checks the others.  Only the code objects' metadata is
read."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NEW = ("ov2_motion_apply", "ov2_motion_apply_batch", "ov2_motion_update", "ov2_motion_update_batch", "ov2_btracker_set_pose",
       "ov2_btracker_get_pose", "ov2_btracker_reset_motion", "ov2_btracker_get_motion", "ov2_btracker_set_keyframe_info",
       "ov2_btracker_track_mono_begin", "ov2_btracker_track_mono_end", "ov2_btracker_track_mono")


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
    from ov2slam_amd import motion
    lib = ov2slam_amd.load()
    hdr = open(os.path.join(ROOT, "include", "ov2slam_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in L.SIGNATURES and name + "(" in hdr, name
    for name in ("apply", "apply_batch", "update", "update_batch", "reset_state"):
        assert callable(getattr(motion, name)), name
    for name in ("trackMono", "trackMonoBegin", "trackMonoEnd", "setPose", "getPose", "resetMotion", "getMotion", "setKeyframeInfo"):
        assert callable(getattr(ov2slam_amd.LockstepTracker, name)), name
    assert (L.OV2_KF_FIRST_FRAME, L.OV2_KF_NO_KEYFRAME) == (512, 1024) and "OV2_KF_FIRST_FRAME = 512" in hdr and "OV2_KF_NO_KEYFRAME = 1024" in hdr
    assert lib.ov2_version() == L.OV2_ABI_VERSION == 600 and "#define OV2_ABI_VERSION 600" in hdr
    for words in ("applyMotionModel", "updateMotionModel", "isZero(1.e-5)", "BIT FOR BIT", "prev_time >= 0 && time <= prev_time",
                  "k_mono_apply", "k_mono_pack", "Twc_h == NULL", "it is finite because"):
        assert words in hdr, words
    mk = open(os.path.join(ROOT, "ov2slam_amd", "csrc", "Makefile")).read()
    assert "se3_dev.hpp" in mk
    pg = open(os.path.join(ROOT, "ov2slam_amd", "csrc", "posegraph.hip")).read()
    assert '#include "se3_dev.hpp"' in pg and "pg_log(const PgSE3" not in pg and "struct PgSE3" not in pg        # one copy


def test_header_compiles_as_c_and_the_new_structs_lay_out_like_it(tmp_path):
    from ov2slam_amd import _lib as L
    pairs = (("ov2_motion_state", L.MotionState), ("ov2_track_mono_params", L.TrackMonoParams), ("ov2_track_mono_input", L.TrackMonoInput),
             ("ov2_track_mono_result", L.TrackMonoResult))
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


def test_inputs_are_checked_before_the_context():
    """no GPU here: with a NULL context a call reaches OV2_EINVAL either way, so what is asserted is that nothing is written and that
    an empty batch with a NULL context is refused too (the context is required), while n < 0 and the non-increasing time are named"""
    import ov2slam_amd
    from ov2slam_amd import _lib as L
    from ov2slam_amd import motion
    lib = ov2slam_amd.load()
    S = motion._states([dict(prev_time=1.0, prevTwc=[0, 0, 0, 0, 0, 0, 1], log_relT=np.zeros(6))])
    So = L.MotionState()
    T, t = np.array([0, 0, 0, 0, 0, 0, 1.0]), np.array([1.0])
    To, Ti, rs = np.full(7, 7.25), np.full(7, 7.25), np.full(1, 0x5a, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.ov2_motion_apply_batch(None, 1, S, p(T), p(t), C.byref(So), p(To), p(Ti), p(rs)) == L.OV2_EINVAL
    assert b"prev_time" in lib.ov2_last_error()                       # the time, not the context
    assert lib.ov2_motion_update_batch(None, 1, S, p(T), p(t), C.byref(So)) == L.OV2_EINVAL
    assert b"prev_time" in lib.ov2_last_error()
    t[0] = 2.0
    assert lib.ov2_motion_apply_batch(None, 1, S, p(T), p(t), C.byref(So), p(To), p(Ti), p(rs)) == L.OV2_EINVAL
    assert b"context" in lib.ov2_last_error()
    assert lib.ov2_motion_apply(None, None, None, 0.0, None, None, None, None) == L.OV2_EINVAL
    assert lib.ov2_motion_update(None, None, None, 0.0, None) == L.OV2_EINVAL
    assert lib.ov2_motion_apply_batch(None, -1, None, None, None, None, None, None, None) == L.OV2_EINVAL
    assert lib.ov2_motion_update_batch(None, -1, None, None, None, None) == L.OV2_EINVAL
    assert (To == 7.25).all() and (Ti == 7.25).all() and rs[0] == 0x5a and So.prev_time == 0.0


def test_rejected_without_a_tracker():
    import ov2slam_amd
    from ov2slam_amd import _lib as L
    lib = ov2slam_amd.load()
    T, s = np.array([0, 0, 0, 0, 0, 0, 1.0]), L.MotionState()
    assert lib.ov2_btracker_set_pose(None, 0, T.ctypes.data_as(C.c_void_p)) == L.OV2_EINVAL
    assert lib.ov2_btracker_get_pose(None, 0, T.ctypes.data_as(C.c_void_p)) == L.OV2_EINVAL
    assert lib.ov2_btracker_reset_motion(None, 0) == L.OV2_EINVAL
    assert lib.ov2_btracker_get_motion(None, 0, C.byref(s)) == L.OV2_EINVAL
    assert lib.ov2_btracker_set_keyframe_info(None, 0, 1, 2.0, 3) == L.OV2_EINVAL
    assert lib.ov2_btracker_track_mono_begin(None, 1, None, 0, None, None, None, None, 1, None, None) == L.OV2_EINVAL
    assert lib.ov2_btracker_track_mono_end(None, None, None, None, None, None, None) == L.OV2_EINVAL
    assert lib.ov2_btracker_track_mono(None, 1, None, 0, None, None, None, None, 1, None, None, None, None, None, None, None, None) == L.OV2_EINVAL
    assert (T == [0, 0, 0, 0, 0, 0, 1.0]).all() and s.prev_time == 0.0


def test_reset_state():
    from ov2slam_amd import motion
    s = motion.reset_state()
    assert s["prev_time"] == -1.0 and np.array_equal(s["prevTwc"], [0, 0, 0, 0, 0, 0, 1]) and not s["log_relT"].any()
    s2 = motion.reset_state(dict(prev_time=3.0, prevTwc=[1, 2, 3, 0, 0, 0, 1], log_relT=np.ones(6)))
    assert s2["prev_time"] == -1.0 and np.array_equal(s2["prevTwc"], [1, 2, 3, 0, 0, 0, 1]) and not s2["log_relT"].any()      # reset() keeps prevTwc_


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_new_kernels_use_no_scratch():
    for name, kernels in (("motion", (("k_motion_apply", 0), ("k_motion_update", 0))), ("mono", (("k_mono_apply", 0), ("k_mono_pack", 32)))):
        res = _resources(name)
        assert len(res) == 2, sorted(res)
        for k, lds in kernels:                                       # the pack: four wavefronts' counts of a round, two sets
            r = _of(res, k)
            print(k, "vgpr", r["next_free_vgpr"], "sgpr", r["next_free_sgpr"], "lds", r["group_segment_fixed_size"])
            assert r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] == lds, (k, r)
            assert r["next_free_vgpr"] <= 128, (k, r)                # a lane per item (the pack: its thread 0): four wavefronts per SIMD


# (VGPRs, LDS bytes) of the commit before this one, from that commit's own build (the kernels are those of DESIGN 4.12, 4.17 and 4.22)
PARENT = {"posegraph": {"k_pg_solve": (308, 512), "k_pg_apply": (62, 0)},
          "fkf": {"k_fkf_parallax": (97, 32824), "k_fkf_sampson": (18, 0)},
          "frameepi": {"k_epif_pack": (36, 32), "k_epif_apply": (10, 0)}}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("name", sorted(PARENT))
def test_surrounding_kernels_keep_their_resources(name):
    res = _resources(name)
    assert len(res) == len(PARENT[name]), sorted(res)
    for k, (vgpr, lds) in PARENT[name].items():
        r = _of(res, k)
        assert (r["next_free_vgpr"], r["group_segment_fixed_size"], r["private_segment_fixed_size"]) == (vgpr, lds, 0), (k, r)


LAYOUT_SRC = r"""
#include <cstdio>
#include "trackb_layout.hpp"
int main()
{
    printf("const %d %d %d\n", BT_MOTION_STATE_BYTES, BT_FKF_ITEM_BYTES, BT_KF_DEC_BYTES);
    const int cases[][2] = {{1, 1}, {3, 64}, {11, 308}, {4096, 308}, {65535, 2048}};
    for (auto &c : cases) {
        const BtMonoLayout L = bt_mono_layout(c[0], c[1]);
        printf("%d %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", c[0], c[1], L.n_tm, L.n_id,
               L.n_ba, L.n_in, L.n_pT, L.n_sa, L.n_su, L.n_dec, L.n_nc, L.n_rs, L.mono_bytes, L.r_T, L.r_st, L.r_kt, L.r_ki, L.res_bytes, L.w_it,
               L.w_lm, L.w_px, L.w_un, L.w_bv, L.w_3d, L.work_bytes);
    }
    return 0;
}
"""


def test_mono_layout(tmp_path):
    """bt_mono_layout against the restatement below: the documented order and sizes, 256-byte starts, no section reaching into the next,
    the upload prefix of the I/O block ending where its download suffix begins; the four older layouts are tests/test_lockstep_layout.py's"""
    cpp, exe = tmp_path / "t.cpp", tmp_path / "t"
    cpp.write_text(LAYOUT_SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "ov2slam_amd", "csrc"), str(cpp), "-o", str(exe)])
    lines = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    assert lines[0].split() == ["const", "112", "176", "48"]
    up = lambda v: (v + 255) & ~255
    assert len(lines) == 6
    for line in lines[1:]:
        v = [int(x) for x in line.split()]
        B, nm, got = v[0], v[1], v[2:]
        slots = B * nm

        def chain(sizes):
            offs, o = [], 0
            for n in sizes:
                offs.append(o)
                o = up(o + n)
            return offs, o
        io, io_total = chain([8 * B, 4 * B, 4 * B, 56 * B, 112 * B, 112 * B, 48 * B, 4 * B, B])
        res, res_total = chain([56 * B, 112 * B, 8 * B, 16 * B])
        work, work_total = chain([176 * B, 4 * slots, 8 * slots, 8 * slots, 24 * slots, slots])
        n_in = io[3]                                                  # the three inputs, then the results
        want = io[:3] + [n_in] + io[3:] + [io_total] + res + [res_total] + work + [work_total]
        assert got == want, (B, nm, got, want)
        assert all(o % 256 == 0 for o in want)
