"""The host plan of the fused strip kernel's LUT computation (ov2slam_amd/csrc/clahe_plan.hpp): which geometries take the row form
of the histograms (whole image rows into 16-bit counters, two tiles per dword) and how much LDS the work-group gets.  The header
is plain C++; it is compiled here with g++ like tests/test_lk_plan.py does for its header.

The row form's conditions, one refusal each: aligned source rows, tw * th < 65536 (a counter half), tw >= 12 (a lane's 12 bytes
touch at most two tiles), the REFLECT_101 padding mirrors into the last tile column / row itself, one LUT wavefront, and an LDS
size that keeps as many work-groups resident on a CU as the tile form's.  The last block pins which of the geometries of
tests/test_gpu_clahe_rowhist.py run the row form, so that a change of the plan cannot silently empty that test."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cstdio>
#include "clahe_plan.hpp"
// the launcher's strip and LUT wavefront counts (ov2_launch_clahe)
static int strips(int w) { const int ndw = (w + 3) / 4; return ndw <= 64 ? 1 : 2 + (ndw - 126 + 61) / 62; }
static int nlut(int tiles_x, int nstrips) { int n = (tiles_x + 7) / 8; if (n > 10 - nstrips) n = 10 - nstrips; if (n < 1) n = 1; return tiles_x <= 16 ? 1 : n; }
static bool row(int w, int h, int tx, int ty, bool al = true) { const int s = strips(w); return ov2_clahe_row_form(w, h, tx, ty, al, s, nlut(tx, s)); }
#define CHECK(c) do { if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); return 1; } } while (0)
int main()
{
    int tw, th;
    ov2_clahe_tile_size(752, 480, 15, 9, &tw, &th);
    CHECK(tw == 51 && th == 54);
    ov2_clahe_tile_size(750, 480, 15, 9, &tw, &th);          // one side divides, the other does not: both are extended
    CHECK(tw == 51 && th == 54);
    ov2_clahe_tile_size(256, 64, 16, 2, &tw, &th);
    CHECK(tw == 16 && th == 32);

    CHECK(row(752, 480, 15, 9));                              // EuRoC
    CHECK(strips(752) == 3 && nlut(15, 3) == 1);
    CHECK(ov2_clahe_lds_tile_form(15, 3, 1) == 31360);
    CHECK(ov2_clahe_lds_row_form(15) == 32512 && ov2_clahe_lds_row_form(15) <= 32768);
    CHECK(ov2_clahe_lds_fused(true, 15, 3, 1) == 32512 && ov2_clahe_lds_fused(false, 15, 3, 1) == 31360);
    CHECK(ov2_clahe_resident(31360, 4) == 5 && ov2_clahe_resident(32512, 4) == 5 && ov2_clahe_resident(32769, 4) == 4);

    CHECK(!row(752, 480, 15, 9, false));                      // unaligned source
    CHECK(!row(1024, 1024, 4, 4));                            // tw * th = 256 * 256 = 65536: one more than a counter half holds
    CHECK(row(1024, 1020, 4, 4));                             // 256 * 255: fits
    CHECK(row(1024, 512, 4, 4));                              // 256 * 128 = 32768
    CHECK(!row(110, 58, 10, 2));                              // tw = 11
    CHECK(row(120, 58, 10, 2));                               // tw = 12
    CHECK(!row(100, 60, 9, 2));                               // tw = 12, tiles end at 108: columns 100..107 mirror 98..91 < 96, the neighbour
    CHECK(!row(200, 50, 4, 7));                               // th = 8, tiles end at 56: rows 50..55 mirror 48..43 < 48
    CHECK(!row(1241, 376, 24, 7));                            // KITTI: three LUT wavefronts
    CHECK(nlut(24, strips(1241)) == 3);
    CHECK(!ov2_clahe_row_form(752, 480, 15, 9, true, 3, 2));  // two LUT wavefronts
    CHECK(!row(256, 64, 16, 2));                              // 8 pair blocks beside one strip: 34048 B leave 4 work-groups where 30848 B leave 5
    CHECK(ov2_clahe_resident(34048, 2) == 4 && ov2_clahe_resident(30848, 2) == 5);

    // tests/test_gpu_clahe_rowhist.py: its geometries that run the row form (sources there are aligned)
    CHECK(row(64, 8, 2, 1) && row(103, 57, 3, 2) && row(264, 100, 5, 2) && row(376, 240, 7, 4) && row(200, 60, 4, 4) && row(1024, 64, 8, 2));
    CHECK(row(240, 64, 15, 2));                               // eight pair blocks, the last one half used, tile edges on dword edges
    printf("OK\n");
    return 0;
}
"""


def test_clahe_plan_row_form_choice_and_lds(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text(SRC)
    exe = tmp_path / "t"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "ov2slam_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "OK", out.stdout + out.stderr
