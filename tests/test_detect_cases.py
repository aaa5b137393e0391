"""The scenes of tests/detect_cases.py on the CPU oracle alone: every geometry and branch that tests/test_gpu_detect_cases.py means to
compare is populated.  These are conditions on the cases, not measurements of the code: a seed that misses one is changed, never the
condition.  `pytest -s` prints the table of counts."""
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import detect_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CLASSES = {"<=36": [c for c in DC.CELLS if c <= 36], "37..52": [c for c in DC.CELLS if 37 <= c <= 52], ">=53": [c for c in DC.CELLS if c >= 53]}


def _add(tot, k):
    for a, b in k.items():
        tot[a] = tot.get(a, 0) + b


@functools.lru_cache(maxsize=None)
def _cell_counts(cell):
    """the oracle's counts of one cell size, summed over its sweep scenes; the restated selections are the oracle's own results"""
    ncell_wg, _ = DC.strip_geometry(cell)
    ss, fa = dict(scenes=0, points=0, free_mult=0, free_nonmult=0, q_down=0, q_up=0, q_same=0), dict(th_down=0, th_up=0, th_same=0, tie_diff=0)
    for s in DC.sweep(cell):
        pts, k = DC.trace_singlescale(s)
        ref, q = DC.oracle_singlescale(s, False)
        assert np.array_equal(pts, ref), s["name"]
        sub, q2 = DC.oracle_singlescale(s, True)
        assert len(sub) == len(ref) and q2 == q
        _add(ss, k)
        ss["scenes"] += 1; ss["points"] += len(ref)
        free = k["cells"] - k["occupied"]
        ss["free_mult" if free % ncell_wg == 0 else "free_nonmult"] += 1
        ss["q_down" if q < s["quality"] else ("q_up" if q > s["quality"] else "q_same")] += 1
        assert q in (s["quality"], s["quality"] / 2.0, s["quality"] * 1.5)
        for mode in (DC.MASK_AS_EXECUTED, DC.MASK_INTENDED):
            pts, k = DC.trace_fast(s, mode)
            ref, th = DC.oracle_fast(s, mode, DC.TIE_SCAN_ORDER)
            assert np.array_equal(pts, ref), (s["name"], mode)
            lib, th2 = DC.oracle_fast(s, mode, DC.TIE_LIBSTDCXX)
            assert len(lib) == len(ref) and th2 == th
            _add(fa, k)
            fa["tie_diff"] += int((lib != ref).any(axis=1).sum())
            fa["th_down" if th < s["fast_th"] else ("th_up" if th > s["fast_th"] else "th_same")] += 1
            assert th in (s["fast_th"], int(s["fast_th"] * 0.66), int(s["fast_th"] * 1.5))
    return ss, fa


@pytest.mark.parametrize("cls", list(CLASSES))
def test_sweep_populates_the_branches(oracle, capsys, cls):
    cs_tot, fa_tot = {}, {}
    lines = []
    for cell in CLASSES[cls]:
        ss, fa = _cell_counts(cell)
        n, k = DC.strip_geometry(cell)
        lines.append("  cell %2d strip (%d,%d): %2d scenes, %4d points, %4d occupied, %3d skipped, free %% n == 0 in %d / != 0 in %d, %3d primaries, "
                     "%3d secondaries (%3d written, truncated %d x, absent %d x), roi %3d, quality %4d, mask-decided %2d, zero cells %4d, column ties %2d, q -/+/= %d/%d/%d"
                     " | FAST %4d points, %3d skipped, sort cells %3d, tied %2d, tie orders differ %2d, weak %4d, th -/+/= %d/%d/%d"
                     % (cell, n, k, ss["scenes"], ss["points"], ss["occupied"], ss["skipped"], ss["free_mult"], ss["free_nonmult"], ss["primaries"],
                        ss["secondaries"], ss["sec_written"], ss["sec_truncated"], ss["sec_absent_full"], ss["roi_rejected"], ss["q_rejected"],
                        ss["mask_decided"], ss["zero_cells"], ss["column_ties"], ss["q_down"], ss["q_up"], ss["q_same"], fa["points"], fa["skipped"], fa["sort_cells"],
                        fa["tie_cells"], fa["tie_diff"], fa["weak"], fa["th_down"], fa["th_up"], fa["th_same"]))
        # ---- per cell size, summed over the scenes ----
        assert ss["points"] > 0 and fa["points"] > 0, cell
        assert ss["occupied"] > 0, cell
        assert ss["skipped"] > 0 and fa["skipped"] > 0, cell
        assert ss["free_mult"] > 0, cell
        assert ss["column_ties"] > 0, cell                          # equal maxima in one column of an accepted cell
        assert ss["free_nonmult"] > 0 or n == 1, cell                # (one cell per work-group: every count is a multiple)
        _add(cs_tot, ss); _add(fa_tot, fa)
    with capsys.disabled():
        print("\n" + "\n".join(lines))
        print("  class %s: %s | FAST %s" % (cls, cs_tot, fa_tot))
    # ---- per k_grid_select cell class ----
    assert cs_tot["mask_decided"] >= 5
    assert cs_tot["sec_written"] > 0 and cs_tot["sec_truncated"] > 0 and cs_tot["sec_absent_full"] > 0
    assert cs_tot["roi_rejected"] > 0 and cs_tot["q_rejected"] > 0 and cs_tot["zero_cells"] > 0
    assert cs_tot["q_down"] > 0 and cs_tot["q_up"] > 0 and cs_tot["q_same"] > 0
    assert fa_tot["th_down"] > 0 and fa_tot["th_up"] > 0 and fa_tot["th_same"] > 0
    assert fa_tot["tie_cells"] > 0 and fa_tot["tie_diff"] > 0       # more than 16 kept corners with tied best scores: the emulated sort decides
    assert oracle.fast_tie_sort_fallbacks() == 0


def test_every_geometry_and_select_instance_is_reached():
    geos = {DC.strip_geometry(c) for c in DC.CELLS}
    waves = {k for _, k in geos}
    assert waves == set(range(1, 9)), waves
    assert len(geos) == 23
    assert DC.strip_geometry(64) == (6, 7) and DC.strip_geometry(63) == (7, 8) and DC.strip_geometry(35) == (5, 3)
    # the 512-thread groups (158 .. 163 KB of LDS); cell 64 would need 165888 B for them and runs 6 cells on 7 wavefronts (145152 B)
    assert {c for c in DC.CELLS if DC.strip_geometry(c)[1] == 8} == {61, 62, 63}
    assert DC.strip_lds(63, 8) == 163296 and DC.strip_lds(64, 8) == 165888 and DC.strip_lds(64, 7) == 145152
    assert all(DC.strip_geometry(c, 0) == DC.strip_geometry(c, 544) for c in DC.CELLS)
    # a cell boundary inside a wavefront's carried columns: owned columns per wavefront that are no multiple of the cell
    assert any((n * c + k - 1) // k % c for c in DC.SOBEL_CELLS for n, k in [DC.strip_geometry(c)] if k > 1)
    single = {DC.select_instance(m, c) for m in (0, 1) for c in DC.CELLS}
    batch = {DC.select_instance(m, c, DC.BATCH_ITEMS) for m in (0, 1) for c in DC.BATCH_CELLS}
    assert len(single) == 6 and len(batch) == 6 and not single & batch
    # the strip rule ncells * items >= 2048 holds and fails among the batch cells; more cell rows than wavefronts (16, or 8 in batches)
    w, h = DC.MAIN
    rule = {c: (w // c) * (h // c) * DC.BATCH_ITEMS >= 2048 for c in DC.BATCH_CELLS}
    assert rule[8] and rule[36] and not rule[53] and not rule[64]
    assert h // 8 > 16 and h // 12 > 8 and h // 8 > 8


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_strip_kernel_static_lds_is_what_the_geometries_assume(tmp_path):
    """a device-only compile of detect.hip for gfx950: k_mineig_strip's static LDS is DC.STRIP_STATIC_LDS, with which cell 63 still fits
    7 cells on 8 wavefronts and cell 64 does not; and each of the twelve k_grid_select instances stays within the static LDS that
    detect_plan.hpp's det_select_lds leaves free for it (the bound is printed from the header by a g++ program, not restated here)"""
    csrc = os.path.join(ROOT, "ov2slam_amd", "csrc")
    src = os.path.join(csrc, "detect.hip")
    out = str(tmp_path / "detect.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "--cuda-device-only", "-S", src, "-o", out],
                   check=True, capture_output=True)
    kernels = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", open(out).read(), re.S)
    fixed = {name: int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1)) for name, body in kernels}
    blocks = [name for name in fixed if "k_mineig_strip" in name]
    assert len(blocks) == 1
    static = fixed[blocks[0]]
    assert static == DC.STRIP_STATIC_LDS
    assert DC.strip_lds(63, 8) + static <= 160 * 1024 < DC.strip_lds(64, 8) + static
    (tmp_path / "bound.cpp").write_text('#include <cstdio>\n#include "detect_plan.hpp"\nint main() { printf("%d\\n", DET_SELECT_STATIC_LDS); return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-I", csrc, str(tmp_path / "bound.cpp"), "-o", str(tmp_path / "bound")])
    bound = int(subprocess.run([str(tmp_path / "bound")], capture_output=True, text=True, check=True).stdout)
    select = {name: b for name, b in fixed.items() if "k_grid_select" in name}
    # <MODE, MAXROW, CHUNKS, NT> as the mangled name spells it: ILi0ELi36ELi1ELi1024EE
    inst = {tuple(int(v) for v in re.search(r"k_grid_selectILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EE", name).groups()) for name in select}
    assert inst == {DC.select_instance(m, c, i) for m in (0, 1) for c in DC.CELLS for i in (1, 64)} and len(select) == 12
    assert all(0 < b <= bound for b in select.values()), (select, bound)


@pytest.mark.parametrize("cell", DC.BORDER_CELLS)
def test_border_shapes(oracle, capsys, cell):
    scenes = DC.border_scenes(cell)
    sizes = {(s["w"], s["h"]) for s in scenes}
    assert {w % cell for w, _ in sizes} >= {0, 1, 2, cell - 1} and {h % cell for _, h in sizes} >= {0, 1, 2, cell - 1}
    assert any(h // cell == 1 and w // cell > 1 for w, h in sizes) and any(w // cell == 1 and h // cell > 1 for w, h in sizes)
    tot, empty = {}, 0
    for s in scenes:
        pts, k = DC.trace_singlescale(s)
        ref, _ = DC.oracle_singlescale(s, False)
        assert np.array_equal(pts, ref), s["name"]
        fpts, fk = DC.trace_fast(s, DC.MASK_INTENDED)
        assert np.array_equal(fpts, DC.oracle_fast(s, DC.MASK_INTENDED, DC.TIE_SCAN_ORDER)[0]), s["name"]
        if min(s["w"], s["h"]) < cell:                              # smaller than one cell: empty
            assert len(ref) == 0 and len(fpts) == 0 and k["cells"] == 0
            empty += 1
        _add(tot, k); tot["fast_points"] = tot.get("fast_points", 0) + len(fpts)
    with capsys.disabled():
        print("\n  border shapes, cell %d: %d shapes, %s" % (cell, len(scenes), tot))
    assert empty == 2 and tot["skipped"] > 0 and tot["primaries"] > 0 and tot["fast_points"] > 0 and tot["occupied"] > 0
    assert tot["sec_absent_full"] > 0 or cell == 8                  # (at cell 8 the ROI's 5 px margin rejects primaries of the border cells)


def test_keypoint_lists_hold_what_they_claim():
    w, h = DC.MAIN
    for cell in (8, 35, 64):
        s = DC.scene("texture", cell, "mixed")
        p = s["cur"].astype(np.float64)
        nw, nh = w // cell, h // cell
        assert ((p[:, 0] % cell == 0) & (p[:, 0] > 0)).any() or nw <= 4        # on a cell boundary
        assert (p % 1 == 0.5).all(axis=1).any()                                 # .5 coordinates
        assert (p[:, 0] < 0).any() and (p[:, 1] < 0).any() and (p[:, 0] >= w).any() and (p[:, 1] >= h).any()
        if nw * cell < w:
            assert ((p[:, 0] >= nw * cell) & (p[:, 0] < w)).any()
        if nh * cell < h:
            assert ((p[:, 1] >= nh * cell) & (p[:, 1] < h)).any()
        assert len(np.unique(p, axis=0)) < len(p)                               # a duplicate
        occ = DC.occupancy(s)
        assert 0 < occ.sum() < occ.size
    assert len(DC.scene("texture", 8, "many", seed=4)["cur"]) > 1024
    assert DC.occupancy(DC.scene("texture", 35, "all", fast_th=40)).all()
    for cell in DC.CELLS:
        mult, non = DC.occupy_counts(cell)
        assert DC.occupancy(DC.scene("halfconst", cell, "occupy:%d" % mult)).sum() == mult
        if non is not None:
            assert DC.occupancy(DC.scene("texture", cell, "occupy:%d" % non, quality=DC.Q_MID, seed=3)).sum() == non


def test_batches_cycle_through_counts_and_states():
    for cell in DC.BATCH_CELLS:
        imgs, which, cur, ncur, q, th = DC.batch(cell)
        ncells = (DC.MAIN[0] // cell) * (DC.MAIN[1] // cell)
        assert len(imgs) == 5 and len(which) == DC.BATCH_ITEMS == len(ncur) and set(which) == set(range(5))
        assert ncur.min() == 0 and ncur.max() == ncells and len(set(ncur.tolist())) >= 3 and cur.shape[1] > ncells
        assert len(set(q.tolist())) >= 5 and len(set(th.tolist())) >= 5
        n_ss = sum(len(DC.oracle_singlescale(DC.batch_item_scene(cell, b), True)[0]) for b in range(DC.BATCH_ITEMS))
        n_f = sum(len(DC.oracle_fast(DC.batch_item_scene(cell, b), DC.MASK_INTENDED, DC.TIE_LIBSTDCXX, True)[0]) for b in range(DC.BATCH_ITEMS))
        assert n_ss > 100 and n_f > 100, (cell, n_ss, n_f)


def test_cases_are_cached():
    a, b = DC.scene("noise", 35, "mixed", "cut", seed=1), DC.scene("noise", 35, "mixed", "cut", seed=1)
    assert a is b and not a["img"].flags.writeable and not a["cur"].flags.writeable
    r1, r2 = DC.oracle_singlescale(a, True), DC.oracle_singlescale(a, True)
    assert r1[0] is r2[0] and not r1[0].flags.writeable
    assert DC.sweep(35) is DC.sweep(35)
