"""The host-only helpers of the frame-versus-keyframe C++ adapter (ov2slam_amd/host/visual_front_end.hpp: the sort of the keyframe
side by lmid, the packing of ov2_fkf_item) in a stand-alone program of their own, built with AddressSanitizer and
UndefinedBehaviorSanitizer and run on the CPU (tests/cpp/kfreq_sort_check.cpp); nothing sanitised is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sort_and_pack_helpers_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "kfreq_sort_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "kfreq_sort_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "kfreq_sort_check ok" in r.stdout, r.stdout + r.stderr
