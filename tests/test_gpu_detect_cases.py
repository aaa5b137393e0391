"""ov2_detect_singlescale / ov2_detect_grid_fast and their batch forms (csrc/detect.hip) against oracle.detect_singlescale and
oracle.detect_grid_fast on the scenes of tests/detect_cases.py, whose branch population tests/test_detect_cases.py asserts on the
oracle alone.  Everything bit for bit: the points as raw float32 bits, the adapted quality / FAST threshold as numbers.  Every cell
size 8..64 (all strip geometries of k_mineig_strip, all twelve k_grid_select instances), both response kernels, both mask modes and
tie orders, the border shapes around the in-image test, both Sobel-dy orders, a padded host image, and 70-item batches."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ov2slam_amd
from ov2slam_amd import _lib as L

from tests import detect_cases as DC

pytestmark = pytest.mark.gpu

GROUPS = [DC.CELLS[i::8] for i in range(8)]                           # small and large cells in every group: even run times
GROUP_IDS = ["cells%d+8k" % g[0] for g in GROUPS]
STRIP = {"cell": 0, "strip": 1}


@pytest.fixture(params=list(STRIP))
def mineig_kernel(request, gpu_ctx):
    """both response kernels of detectSingleScale, pinned through OV2_OPT_DETECT_STRIP: one wavefront per cell (k_mineig_cells) and the
    strip of free cells (k_mineig_strip); left alone the library picks by launch size and single images would only see the first"""
    with gpu_ctx.options(detect_strip=STRIP[request.param]):
        yield request.param


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what):
    assert got.shape == want.shape, "%s: %d points, the oracle has %d" % (what, len(got), len(want))
    bad = np.nonzero((_bits(got) != _bits(want)).any(axis=1))[0]
    assert len(bad) == 0, "%s: %d of %d points differ, first %d: %s / %s" % (what, len(bad), len(got), bad[0], got[bad[0]], want[bad[0]])


def _run_singlescale(ctx, s, subpix, sobel_dy=0):
    fx = ov2slam_amd.FeatureExtractor(ctx, dmaxquality=s["quality"])
    got = fx.detectSingleScale(s["img"], s["cell"], s["cur"], s["roi"], subpix=subpix)
    want, q = DC.oracle_singlescale(s, subpix, sobel_dy)
    _same(got, want, "%s subpix %d" % (s["name"], subpix))
    assert fx.dmaxquality_ == q, (s["name"], fx.dmaxquality_, q)
    return len(want)


def _run_fast(ctx, s, mode, tie, subpix):
    fx = ov2slam_amd.FeatureExtractor(ctx, nfast_th=s["fast_th"], mask_mode=mode)
    got = fx.detectGridFAST(s["img"], s["cell"], s["cur"], subpix=subpix)
    want, th = DC.oracle_fast(s, mode, tie, subpix)
    _same(got, want, "%s mask mode %d tie order %d subpix %d" % (s["name"], mode, tie, subpix))
    assert fx.nfast_th_ == th, (s["name"], fx.nfast_th_, th)
    return len(want)


@pytest.mark.parametrize("cells", GROUPS, ids=GROUP_IDS)
def test_singlescale_every_cell(gpu_ctx, oracle, mineig_kernel, cells):
    for cell in cells:
        n = 0
        for s in DC.sweep(cell):
            for subpix in (False, True):
                n += _run_singlescale(gpu_ctx, s, subpix)
        assert n > 0, cell


@pytest.mark.parametrize("tie", [L.OV2_FAST_TIE_SCAN_ORDER, L.OV2_FAST_TIE_LIBSTDCXX], ids=["scan", "libstdcxx"])
@pytest.mark.parametrize("cells", GROUPS, ids=GROUP_IDS)
def test_grid_fast_every_cell(gpu_ctx, oracle, cells, tie):
    with gpu_ctx.options(fast_tie=tie):
        for cell in cells:
            n = 0
            for i, s in enumerate(DC.sweep(cell)):
                for mode in (L.OV2_MASK_AS_EXECUTED, L.OV2_MASK_INTENDED):
                    n += _run_fast(gpu_ctx, s, mode, tie, subpix=False)
                    if i in (0, 3):
                        _run_fast(gpu_ctx, s, mode, tie, subpix=True)
            assert n > 0, cell
    assert oracle.fast_tie_sort_fallbacks() == 0


@pytest.mark.parametrize("cell", DC.BORDER_CELLS)
def test_border_shapes(gpu_ctx, oracle, mineig_kernel, cell):
    """widths and heights on both sides of x0 + cell < w - 1, one cell row, one cell column, an image smaller than one cell"""
    n = 0
    for s in DC.border_scenes(cell):
        n += _run_singlescale(gpu_ctx, s, False) + _run_singlescale(gpu_ctx, s, True)
        if mineig_kernel == "cell":                                  # (the option does not reach the FAST kernels: once)
            for mode in (L.OV2_MASK_AS_EXECUTED, L.OV2_MASK_INTENDED):
                n += _run_fast(gpu_ctx, s, mode, gpu_ctx.get_option(L.OV2_OPT_FAST_TIE), subpix=True)
    assert n > 0


@pytest.mark.parametrize("order", [L.OV2_SOBEL_DY_OPENCV_ROWFILTER, L.OV2_SOBEL_DY_EXACT_SUM], ids=["rowfilter", "exact_sum"])
def test_sobel_dy_orders_under_the_strip_kernel(gpu_ctx, oracle, order):
    """cells 8, 17 (7 cells on 2 wavefronts), 37 (8 on 5), 52 (8 on 7) and 63 (7 on 8): a cell boundary inside a wavefront's carried columns"""
    with gpu_ctx.options(detect_strip=1, sobel_dy_order=order):
        for cell in DC.SOBEL_CELLS:
            assert sum(_run_singlescale(gpu_ctx, s, True, sobel_dy=order) for s in DC.sweep(cell)[:5]) > 0, cell


def test_padded_host_image(gpu_ctx, oracle, mineig_kernel):
    """a host image whose row stride exceeds its width, through the C ABI (the wrappers always pass stride = w)"""
    lib = gpu_ctx.lib
    for s in (DC.sweep(35)[0], DC.sweep(58)[4]):
        w, h, cell = s["w"], s["h"], s["cell"]
        stride = w + 37
        pad = np.full((h, stride), 0xAB, np.uint8)
        pad[:, :w] = s["img"]
        cur = np.ascontiguousarray(s["cur"], np.float32)
        ncells = (w // cell) * (h // cell)
        out = np.zeros((2 * ncells, 2), np.float32); n = C.c_int(0); q = C.c_double(s["quality"])
        roi = (C.c_int * 4)(*s["roi"])
        L.check(lib.ov2_detect_singlescale(gpu_ctx.h, pad.ctypes.data_as(C.c_void_p), w, h, stride, cell, cur.ctypes.data_as(C.c_void_p), len(cur),
                                           roi, C.byref(q), 1, out.ctypes.data_as(C.c_void_p), C.byref(n)))
        want, rq = DC.oracle_singlescale(s, True)
        _same(out[:n.value], want, s["name"] + " padded")
        assert q.value == rq and len(want) > 0
        for mode in (L.OV2_MASK_AS_EXECUTED, L.OV2_MASK_INTENDED):
            out = np.zeros((ncells, 2), np.float32); n = C.c_int(0); th = C.c_int(s["fast_th"])
            L.check(lib.ov2_detect_grid_fast(gpu_ctx.h, pad.ctypes.data_as(C.c_void_p), w, h, stride, cell, cur.ctypes.data_as(C.c_void_p), len(cur),
                                             C.byref(th), mode, 1, out.ctypes.data_as(C.c_void_p), C.byref(n)))
            want, rth = DC.oracle_fast(s, mode, gpu_ctx.get_option(L.OV2_OPT_FAST_TIE), True)
            _same(out[:n.value], want, s["name"] + " padded, FAST")
            assert th.value == rth and len(want) > 0


_BATCH_SCRIPT = r"""
import sys, numpy as np
import torch
torch.cuda.init()
sys.path.insert(0, sys.argv[1])
import ov2slam_amd
from ov2slam_amd import _lib as L
from tests import detect_cases as DC
cell = int(sys.argv[2])
ctx = ov2slam_amd.Context(0)
W, H = DC.MAIN
imgs, which, cur, ncur, q0, th0 = DC.batch(cell)
B, cur_cap = len(which), cur.shape[1]
ncells = (W // cell) * (H // cell)
P = ov2slam_amd.Pyramid(ctx, W, H, 9, 0, batch=B).build(np.stack([imgs[i] for i in which]))
ctx.sync()
d_cur = torch.from_numpy(cur).cuda(); d_n = torch.from_numpy(ncur).cuda()
roi = DC.usual_roi(W, H)
tie = ctx.get_option(L.OV2_OPT_FAST_TIE)
PAD = 5                                                               # slots beyond the capacity: must stay untouched
def same(out, n, b, want, what):
    assert n[b] == len(want), (what, "count", b, int(n[b]), len(want))
    assert np.array_equal(out[b, :n[b]].view(np.uint32), want.view(np.uint32)), (what, "bits", b)
total = 0
# ---- single scale: the library's own choice of response kernel (ncells * items >= 2048 -> the strip kernel), then the strip kernel pinned ----
auto_strip = ncells * B >= 2048
for strip in ((-1,) if auto_strip else (-1, 1)):
    with ctx.options(detect_strip=strip):
        cap = 2 * ncells
        d_out = torch.full((B, cap + PAD, 2), -7.0, dtype=torch.float32, device="cuda")
        q = q0.copy()
        torch.cuda.synchronize()
        n = ov2slam_amd.FeatureExtractor.detectSingleScaleBatch(ctx, P, cell, d_cur.data_ptr(), cur_cap, d_n.data_ptr(), roi, q, d_out.data_ptr(), cap + PAD, subpix=True)
        out = d_out.cpu().numpy()
        for b in range(B):
            want, rq = DC.oracle_singlescale(DC.batch_item_scene(cell, b), True)
            same(out, n, b, want, "singlescale strip %d" % strip)
            assert q[b] == rq, ("quality", b, q[b], rq)
            assert np.all(out[b, cap:] == -7.0), ("slots beyond the capacity", b)
            total += len(want)
# ---- FAST, both mask modes ----
for mode in (L.OV2_MASK_AS_EXECUTED, L.OV2_MASK_INTENDED):
    cap = ncells
    d_out = torch.full((B, cap + PAD, 2), -7.0, dtype=torch.float32, device="cuda")
    th = th0.copy()
    torch.cuda.synchronize()
    n = ov2slam_amd.FeatureExtractor.detectGridFASTBatch(ctx, P, cell, d_cur.data_ptr(), cur_cap, d_n.data_ptr(), th, d_out.data_ptr(), cap + PAD, mask_mode=mode, subpix=True)
    out = d_out.cpu().numpy()
    for b in range(B):
        want, rth = DC.oracle_fast(DC.batch_item_scene(cell, b), mode, tie, True)
        same(out, n, b, want, "fast mode %d" % mode)
        assert th[b] == rth, ("threshold", b, th[b], rth)
        assert np.all(out[b, cap:] == -7.0), ("slots beyond the capacity", b)
        total += len(want)
assert total > 300, total
ctx.close()
print("BATCH_DETECT_CASES_OK")
"""


@pytest.mark.parametrize("cell", DC.BATCH_CELLS)
def test_batch_forms_against_the_oracle(cell):
    """ov2_detect_singlescale_batch_d / ov2_detect_grid_fast_batch_d on 70 items (the 512-thread k_grid_select instances): item by item
    the oracle's points, count and adapted state.  Cell 8 has 25 cell rows on 8 wavefronts; cells 8..37 take the strip kernel by the
    launch-size rule, 52..64 the one-wavefront kernel and then the strip kernel pinned.  Own process: torch owns the device buffers."""
    pytest.importorskip("torch")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _BATCH_SCRIPT, root, str(cell)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "BATCH_DETECT_CASES_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
