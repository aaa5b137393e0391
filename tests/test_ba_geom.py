"""ov2slam_amd/csrc/ba_geom.hpp on the host: the dynamic-LDS sizes, path decisions and launch geometry of the device bundle
adjustment.  tests/cpp/ba_geom_check.cpp sweeps n_opt = 1 .. 1024 against that header alone (no HIP, no GPU)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ba_geom_sizes_paths_and_grids(tmp_path):
    """Whenever ba_small_path holds, the inverse-depth lineariser and the LDS Cholesky are within their limits and nf <= CH_MAX_LDS_N;
    lin_direct switches on exactly where the aggregated large-path lineariser exceeds its limit; lin_waves is the largest of 4, 2, 1
    that fits; ksplit * lm_per_split covers the landmarks, lm_per_split is whole tiles, every grid is at least 1 and a batch's
    per-field maximum is at least every member's (the program prints a FAIL line per violation).  The small / large boundary
    lies between 69 and 70 optimised keyframes: nf = 414 with 124 920 B (lineariser) and 116 544 B (Cholesky), then nf = 420.
    ba_out_layout and ba_batch_header (the blocks of a lock-step batch, written by k_ba_gather_B and read by the host through the
    same function) against the program's own restatement, (n_kf, n_lm, n_res) in {(1,0,0), (1,1,1), (6,40,160), (25,3000,69000)}
    x the four flag values and N in {1, 11, 4096}: every part starts on a multiple of 256 where the restatement puts it and ends
    before the next, the total is the end of the last part, the chi2 / depth-flag parts exist exactly with flags 1 / 2."""
    exe = str(tmp_path / "ba_geom_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "ov2slam_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "ba_geom_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert "FAIL" not in r.stdout and r.returncode == 0, r.stdout[:4000]
    fig = {k: int(v) for k, v in (line.split() for line in r.stdout.splitlines())}
    assert fig["failures"] == 0
    assert fig["last_small"] == 69 and fig["last_small_nf"] == 414 and fig["first_large_nf"] == 420
    assert fig["last_small_lin_lds"] == 124920 and fig["last_small_chol_lds"] == 116544
    # the thresholds the comments of ba.hip / ba_problem.hpp quote
    assert fig["first_lin_direct"] == 583
    assert (fig["last_lin_waves_4"], fig["last_lin_waves_2"], fig["last_lin_waves_1"]) == (202, 320, 451)
    # a 25-keyframe window with every part: 1 536 + 24 064 + 69 120 + 552 192 + 69 120 bytes
    assert fig["out_total_25kf_flags3"] == 716032
