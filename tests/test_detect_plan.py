"""The host plan of the grid detectors (ov2slam_amd/csrc/detect_plan.hpp): strip geometry, k_grid_select instance and LDS bytes, the
launch-size rule, the two scratch layouts, the reference's adaptation rules and the geometry check.  The header is plain C++; a small
program compiled here with g++ (like tests/test_lk_plan.py does for its header) prints what it decides, and every line is compared with
the Python of tests/detect_cases.py -- the tests' own statement of the same decisions -- or with a restatement written below."""
import functools
import os
import subprocess
import tempfile

from tests import detect_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS = 160 * 1024
NO_ROOM = LDS - 1000                 # a static size beside which no strip geometry of any cell fits (the smallest, one cell of 8 on one wavefront, takes 2592 B)
STATICS = (0, DC.STRIP_STATIC_LDS, 544, NO_ROOM)
SHAPES = ((264, 200), (1280, 720))
LAYOUT_CELLS, LAYOUT_ITEMS = (8, 35, 64), (1, 70, 512, 513, 1100)
RULE_CASES = ((2047, 1), (2048, 1), (2049, 1), (1023, 2), (1024, 2), (29, 70), (30, 70), (1, 2047), (1, 2048), (3000000, 1000))

SRC = r"""
#include <cstdio>
#include <cstdlib>
#include "detect_plan.hpp"
int main(int argc, char **argv)
{
    printf("const %d %d %d %d %zu %d %d %d\n", DET_MAX_CELL, DET_CHUNK, DET_SORT_CAP, STRIP_MAX_CELLS, (size_t)DET_LDS_BYTES, DET_SELECT_STATIC_LDS,
           DET_CAND_BYTES, DET_SELECT_OUT_BYTES);
    for (int a = 1; a < argc; a++)
        for (int cell = 8; cell <= 64; cell++) {
            const DetStrip g = det_strip_geometry(cell, atoi(argv[a]));
            printf("strip %d %d %d %d %d %zu\n", atoi(argv[a]), cell, g.cells, g.waves, g.owned, g.lds);
        }
    for (int cell = 8; cell <= 64; cell++)
        for (int k = 1; k <= 8; k++) printf("striplds %d %d %zu\n", cell, k, det_strip_lds(cell, k));
    const int items[4] = {1, 63, 64, 70};
    for (int cell = 8; cell <= 64; cell++)
        for (int it : items) {
            const DetSelectClass c = DET_SELECT_CLASS[det_select_class(cell)];
            printf("select %d %d %d %d %d\n", cell, it, c.maxrow, c.chunks, det_select_threads(it));
        }
    const int rule[][2] = {RULE_CASES};
    for (auto &r : rule)
        for (int ds = -1; ds <= 1; ds++) printf("rule %d %d %d %d\n", ds, r[0], r[1], (int)det_use_strip(ds, r[0], r[1]));
    const int shapes[][2] = {SHAPE_CASES};
    for (auto &s : shapes)
        for (int cell = 8; cell <= 64; cell++)
            for (int mode = 0; mode < 2; mode++)
                for (int tie = 0; tie < 2; tie++) {
                    int slots = -1;
                    const size_t b = det_select_lds(s[0], s[1], cell, mode, tie == 1, &slots);
                    printf("sellds %d %d %d %d %d %zu %d %d\n", s[0], s[1], cell, mode, tie, b, slots, (int)det_check_geometry(s[0], s[1], cell, mode, tie == 1));
                }
    const int ths[5] = {1, 2, 3, 10, 255}, empties[6] = {0, 10, 11, 12, 40, 41};
    for (int th : ths)
        for (int e : empties)
            for (int k = 0; k <= e; k++) printf("fast %d %d %d %d\n", th, k, e, det_adapt_fast_th(th, k, e));
    const double qs[3] = {1e-3, 2e-2, 10.0};
    const int grids[4][2] = {{100, 0}, {825, 275}, {12, 5}, {12, 12}};
    for (double q : qs)
        for (auto &g : grids)
            for (int n = 0; n <= 2 * g[0]; n++) printf("quality %.17g %d %d %d %.17g\n", q, n, g[0], g[1], det_adapt_quality(q, n, g[0], g[1]));
    const int lcells[3] = {LAYOUT_CELLS}, litems[5] = {LAYOUT_ITEMS}, ncurs[3] = {0, 1, 300};
    for (int cell : lcells)
        for (int mode = 0; mode < 2; mode++) {
            const int ncells = (264 / cell) * (200 / cell);
            for (int ncur : ncurs)
                for (int up = 0; up < 2; up++) {
                    const DetScratch s = det_scratch(264, 200, cell, mode, ncur, up == 1);
                    printf("single %d %d %d %d %zu %zu %zu %zu %zu %zu %zu %zu\n", cell, mode, ncur, up, s.img, s.map, s.cur, s.out, s.so, s.cand, s.free_list, s.total);
                }
            for (int it : litems) {
                const DetBatchScratch s = det_batch_scratch(cell, ncells, mode, it);
                printf("batch %d %d %d %d %d %zu %zu %zu %zu %zu %zu %zu\n", cell, mode, it, s.sets, s.chunk, s.map, s.cand, s.free_list, s.set_bytes, s.so, s.par, s.total);
            }
            printf("outcap %d %d %d\n", mode, ncells, det_out_cap(mode, ncells));
        }
    const int checks[][3] = {{264, 200, 7}, {264, 200, 8}, {264, 200, 64}, {264, 200, 65}, {65535, 7, 8}, {65536, 7, 8}, {7, 32767, 8}, {7, 32768, 8},
                             {65536, 200, 7}, {60000, 10, 16}, {1280, 720, 8}};
    for (auto &c : checks) printf("check %d %d %d %d\n", c[0], c[1], c[2], (int)det_check_geometry(c[0], c[1], c[2], 1, false));
    return 0;
}
"""


def _csv(rows):
    return ", ".join("{%s}" % ", ".join(str(v) for v in r) if isinstance(r, tuple) else str(r) for r in rows)


@functools.lru_cache(maxsize=None)
def plan():
    """every line the program prints, grouped by its first word; numbers as ints (floats where they do not parse as ints)"""
    src = SRC.replace("RULE_CASES", _csv(RULE_CASES)).replace("SHAPE_CASES", _csv(SHAPES))
    src = src.replace("LAYOUT_CELLS", _csv(LAYOUT_CELLS)).replace("LAYOUT_ITEMS", _csv(LAYOUT_ITEMS))
    with tempfile.TemporaryDirectory() as tmp:
        cpp, exe = os.path.join(tmp, "t.cpp"), os.path.join(tmp, "t")
        with open(cpp, "w") as f:
            f.write(src)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "ov2slam_amd", "csrc"), cpp, "-o", exe])
        out = subprocess.run([exe] + [str(s) for s in STATICS], capture_output=True, text=True, timeout=60, check=True).stdout
    rows = {}
    for line in out.splitlines():
        key, *vals = line.split()
        rows.setdefault(key, []).append(tuple(int(v) if v.lstrip("-").isdigit() else float(v) for v in vals))
    return rows


def test_constants():
    (max_cell, chunk, sort_cap, strip_cells, lds, sel_static, cand, so), = plan()["const"]
    assert (max_cell, chunk, sort_cap, strip_cells, lds) == (DC.CELLS[-1], 1024, 512, 8, LDS)
    assert 0 < sel_static <= 1024 and (cand, so) == (16, 56)      # CellCand: 2 ints + 2 floats; SelectOut: 6 ints + 4 ticks of 8 B


def test_strip_geometry_is_the_cases_own():
    rows = plan()["strip"]
    assert len(rows) == len(STATICS) * len(DC.CELLS)
    got = {(st, cell): (n, k, owned, lds) for st, cell, n, k, owned, lds in rows}
    for st in STATICS[:3]:
        for cell in DC.CELLS:
            n, k = DC.strip_geometry(cell, st)
            assert got[st, cell] == (n, k, (n * cell + k - 1) // k, DC.strip_lds(cell, k)), (st, cell)
            assert got[st, cell][3] + st <= LDS and got[st, cell][2] <= 60
    s = DC.STRIP_STATIC_LDS
    assert got[s, 63] == (7, 8, 56, 163296) and got[s, 64] == (6, 7, 55, 145152) and got[s, 35][:2] == (5, 3)
    assert all(got[NO_ROOM, cell] == (0, 0, 0, 0) for cell in DC.CELLS)          # nothing fits
    assert all(b == DC.strip_lds(cell, k) for cell, k, b in plan()["striplds"]) and len(plan()["striplds"]) == 8 * len(DC.CELLS)


def test_select_instance_is_the_cases_own():
    rows = plan()["select"]
    assert len(rows) == 4 * len(DC.CELLS)
    for cell, items, maxrow, chunks, threads in rows:
        for mode in (0, 1):                                       # (the mode is the table's first index: the class and the thread count do not depend on it)
            assert DC.select_instance(mode, cell, items) == (mode, maxrow, chunks, threads), (cell, items)
        assert cell <= maxrow * chunks
    assert {r[1] for r in rows} == {1, 63, 64, 70}
    assert all(cap == (n if mode == 0 else 2 * n) for mode, n, cap in plan()["outcap"])


def test_strip_rule():
    rows = plan()["rule"]
    assert len(rows) == 3 * len(RULE_CASES)
    for ds, ncells, items, strip in rows:
        assert bool(strip) == (ds == 1 or (ds < 0 and ncells * items >= 2048)), (ds, ncells, items)
    auto = {(n, i): s for ds, n, i, s in rows if ds == -1}
    assert auto[2047, 1] == 0 and auto[2048, 1] == 1 and auto[29, 70] == 0 and auto[30, 70] == 1 and auto[3000000, 1000] == 1


def test_select_lds():
    limit = LDS - plan()["const"][0][5]
    area = (512 + 72) * 4
    rows = plan()["sellds"]
    assert len(rows) == len(SHAPES) * len(DC.CELLS) * 4
    zero = fits = 0
    for w, h, cell, mode, tie, total, slots, check in rows:
        nw, nh, wpr = w // cell, h // cell, (w + 31) // 32
        # mask, disc half-widths, candidates, row progress, cell states (padded to words), two more ints per cell
        base = h * wpr * 4 + 64 * 4 + nw * nh * 16 + nh * 4 + (((nh + 1) * (nw + 1) + 3) & ~3) + nw * nh * 8
        sort = mode == 0 and tie == DC.TIE_LIBSTDCXX
        if base > limit or (sort and (limit - base) // area == 0):
            assert (total, slots) == (0, 0), (w, h, cell, mode, tie)
            zero += 1
        else:
            assert (1 <= slots <= 16 and slots == min(16, (limit - base) // area)) if sort else slots == 0, (w, h, cell, mode, tie)
            assert total == base + slots * area and 0 < total <= limit
            fits += 1
        assert (total == 0) == (base > limit) or sort
        assert check == (3 if total == 0 else 0)                  # the geometry check refuses exactly these
    assert zero > 0 and fits > 0
    assert all(r[5] > 0 for r in rows if r[:2] == (264, 200)) and any(r[5] == 0 for r in rows if r[:2] == (1280, 720))


def _fast_rule(th, nbkps, nbempty):                                 # feature_extractor.cpp:546-552: nfast_th_ is an int, *= a double truncates
    if nbkps < 0.5 * nbempty and nbempty > 10:
        return int(th * 0.66)
    if nbkps == nbempty:
        return int(th * 1.5)
    return th


def _quality_rule(q, n, ncells, nboccup):                           # :418-423
    if n < 0.33 * (ncells - nboccup):
        return q / 2.0
    if n > 0.9 * (ncells - nboccup):
        return q * 1.5
    return q


def test_adaptation_rules():
    fast = plan()["fast"]
    for th, nbkps, nbempty, out in fast:
        assert out == _fast_rule(th, nbkps, nbempty), (th, nbkps, nbempty)
    got = {(th, k, e): out for th, k, e, out in fast}
    assert (got[10, 19, 40], got[10, 20, 40], got[10, 20, 41], got[10, 21, 41]) == (6, 10, 6, 10)        # just below and at half of the empty cells
    assert (got[10, 0, 10], got[10, 0, 11], got[10, 10, 10], got[10, 0, 0]) == (10, 6, 15, 15)           # more than 10 empty cells; every empty cell filled
    assert [got[th, 0, 40] for th in (1, 2, 3, 10, 255)] == [0, 1, 1, 6, 168]                            # truncation
    assert [got[th, 40, 40] for th in (1, 2, 3, 10, 255)] == [1, 3, 4, 15, 382]
    qual = plan()["quality"]
    for q, n, ncells, nboccup, out in qual:
        assert out == _quality_rule(q, n, ncells, nboccup), (q, n, ncells, nboccup)
    got = {(q, n, c, o): out for q, n, c, o, out in qual}
    assert [got[2e-2, n, 100, 0] for n in (32, 33, 34, 89, 90, 91)] == [1e-2, 2e-2, 2e-2, 2e-2, 2e-2, 2e-2 * 1.5]       # 0.33 * 100 and 0.9 * 100 round to 33 and 90
    assert [got[1e-3, n, 825, 275] for n in (181, 182, 495, 496)] == [5e-4, 1e-3, 1e-3, 1e-3 * 1.5]       # 550 free cells: 181.5 and 495
    assert got[10.0, 0, 12, 12] == 10.0 and got[10.0, 1, 12, 12] == 15.0                                  # no free cell


def _sections_ok(offsets, sizes, total, aligned):
    """ascending, inside [0, total], no section reaching into the next; `aligned`: which start on a 256-byte boundary"""
    ends = offsets[1:] + [total]
    for i, (o, n, e) in enumerate(zip(offsets, sizes, ends)):
        assert o + n <= e, (i, offsets, sizes, total)
        assert not aligned[i] or o % 256 == 0, (i, offsets)
    assert offsets == sorted(offsets) and offsets[0] == 0


def test_scratch_layouts():
    w, h = DC.MAIN
    cand_b, so_b = plan()["const"][0][6:8]
    rows = plan()["single"]
    assert len(rows) == len(LAYOUT_CELLS) * 2 * 3 * 2
    for cell, mode, ncur, up, img, mp, cur, out, so, cand, free, total in rows:
        ncells = (w // cell) * (h // cell)
        maps = ncells * cell * cell * (1 if mode == 0 else 4)
        # image (uploads only), maps, current keypoints, 2 * ncells output points directly followed by the counters (one copy back), candidates, free list
        _sections_ok([img, mp, cur, out, so, cand, free], [w * h if up else 0, maps, 8 * ncur, 16 * ncells, so_b, cand_b * ncells, 4 * (ncells + 1)], total,
                     [True, True, True, True, False, True, False])
        assert so == out + 16 * ncells and free == cand + cand_b * ncells and total == free + 4 * (ncells + 1) and free % 4 == 0
        assert (mp == 0) == (not up)
    rows = plan()["batch"]
    assert len(rows) == len(LAYOUT_CELLS) * 2 * len(LAYOUT_ITEMS)
    for cell, mode, items, sets, chunk, mp, cand, free, set_bytes, so, par, total in rows:
        ncells = (w // cell) * (h // cell)
        maps = ncells * cell * cell * (1 if mode == 0 else 4)
        assert (sets, chunk) == ((2, 512) if items >= 513 else (1, items))
        _sections_ok([mp, cand, free], [chunk * maps, chunk * cand_b * ncells, chunk * 4 * (ncells + 1)], set_bytes, [True, True, False])
        assert free % 4 == 0 and set_bytes % 256 == 0 and so == sets * set_bytes
        _sections_ok([0, so, par], [sets * set_bytes, items * so_b, items * 8], total, [True, True, True])


def test_geometry_check():
    got = {(w, h, cell): c for w, h, cell, c in plan()["check"]}
    ok, bad_cell, bad_size, bad_mask = 0, 1, 2, 3
    assert got[264, 200, 7] == bad_cell and got[264, 200, 8] == ok and got[264, 200, 64] == ok and got[264, 200, 65] == bad_cell
    # (shapes without a whole cell, so that the mask plays no part)
    assert got[65535, 7, 8] == ok and got[65536, 7, 8] == bad_size and got[7, 32767, 8] == ok and got[7, 32768, 8] == bad_size
    assert got[65536, 200, 7] == bad_cell                           # the cell size is looked at first
    assert got[60000, 10, 16] == ok                                 # no whole cell: an empty result, whatever the mask would take
    assert got[1280, 720, 8] == bad_mask
