"""The host-only helpers of the prior adapters (ov2slam_amd/host/visual_front_end.hpp: the packing of ov2_klt_priors_item;
ov2slam_amd/host/feature_tracker.hpp: the Frame's grid size, the cell offsets and rows built from vgridkps_, the packing of
ov2_stereo_priors_item) in a stand-alone program of their own, built with AddressSanitizer and UndefinedBehaviorSanitizer and run on
the CPU (tests/cpp/priors_table_check.cpp); nothing sanitised is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_index_and_table_helpers_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "priors_table_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "priors_table_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "priors_table_check ok" in r.stdout, r.stdout + r.stderr
