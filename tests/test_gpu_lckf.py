"""The loop closer's keyframe preparation on the GPU (csrc/lckf.hip, ov2_lckf_prepare*) against the numpy specification
(tests/lckf_ref.py, flat()): every output array byte-equal -- the counts, the cut, both corner lists, the valid flags and the
descriptors -- at image sizes around the kernel's tile, with exclusion lists of several lengths, on the synthetic frames with their
literal counts, on the crafted cases with their literals, with lists cut at their capacities, in the batch form against single calls
and on both sides of the scratch chunk boundary, twice in a row, with a custom BRIEF pattern, through the tracker and lock-step
tracker forms, against ov2_describe_brief on the same points, and through the C++ adapter in both orders."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ov2slam_amd
from ov2slam_amd import loop_closer as LC
from tests import lckf_ref as R
from tests.test_lckf_reference import table_rows
from tests.test_lckf_resources import LCKF_TILE_H, LCKF_TILE_W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, U = LCKF_TILE_W, LCKF_TILE_H
SIZES = [(6, 9), (9, 6), (7, 7), (56, 80), (57, 57)] + [(w, h) for w in (T - 1, T, T + 1, 2 * T + 5) for h in (U - 1, U, U + 1, 2 * U + 5)]
ARRAYS = ("all_xy", "all_resp", "kept_xy", "kept_resp", "kept_valid", "kept_desc")


@pytest.fixture(scope="module")
def pattern():
    return R.builtin_pattern()


def _check(got, ref, what=""):
    ok, field = R.same({f: got[f] for f in R.FIELDS}, ref)
    if not ok:
        g, r = np.asarray(got[field]), np.asarray(ref[field])
        raise AssertionError("%s %s differs (shapes %s / %s, dtypes %s / %s): got %s, want %s"
                             % (what, field, g.shape, r.shape, g.dtype, r.dtype, g.reshape(-1)[:24], r.reshape(-1)[:24]))


def _params(p):
    return LC.lckf_params(p["threshold"], p["retain"], p["radius"])


@pytest.mark.parametrize("n_excl", [0, 1, 65, 300])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_byte_equal_against_specification(gpu_ctx, pattern, size, n_excl):
    assert (T, U) == (64, 16) and SIZES[-1] == (133, 37)
    w, h = size
    rng = np.random.default_rng(1000 * w + 10 * h + n_excl)
    img, e = R.make_case(rng, w, h, n_excl, "noise" if (w + h) % 2 else "textured")
    n = len(R.corners(img, 20)[0])
    for retain in sorted({300, max(1, n // 2)}):
        ref = R.flat(img, e, pattern, retain=retain)
        _check(LC.lckf_prepare(gpu_ctx, LC.lckf_params(retain=retain), img, e, want_all=True), ref, "%dx%d retain %d" % (w, h, retain))
        if w < 7 or h < 7:
            assert ref["n_all"] == 0
        if w <= 56 or h <= 56:
            assert ref["n_desc"] == 0


@pytest.mark.parametrize("row", table_rows()[:2], ids=lambda r: r[0])
def test_synthetic_frames_with_their_literal_counts(gpu_ctx, pattern, row):
    name, img, e, (n_nms, n_all, cut, n_kept, n_at_cut, n_desc) = row
    got = LC.lckf_prepare(gpu_ctx, LC.lckf_params(), img, e, want_all=True)
    assert (got["n_all"], got["cut"], got["n_kept"], int((got["kept_resp"] == cut).sum()), got["n_desc"]) == (n_all, cut, n_kept, n_at_cut, n_desc)
    _check(got, R.flat(img, e, pattern), name)
    none = LC.lckf_prepare(gpu_ctx, LC.lckf_params(retain=-1), img, None, want_all=True)
    assert none["n_all"] == none["n_kept"] == n_nms and np.array_equal(none["all_xy"], none["kept_xy"])
    view = np.zeros((img.shape[0], img.shape[1] + 7), np.uint8)                    # a row stride that is no multiple of 4
    view[:, :img.shape[1]] = img
    _check(LC.lckf_prepare(gpu_ctx, LC.lckf_params(), view[:, :img.shape[1]], e, want_all=True), R.flat(img, e, pattern), name + " strided")


@pytest.mark.parametrize("case", R.crafted_cases(T, U), ids=lambda c: c[0])
def test_crafted_cases_byte_equal(gpu_ctx, pattern, case):
    name, img, excl, p, want = case
    got = LC.lckf_prepare(gpu_ctx, _params(p), img, excl, want_all=True)
    assert (got["n_all"], got["cut"], got["n_kept"], got["n_desc"]) == (want["n_all"], want["cut"], want["n_kept"], want["n_desc"]), name
    assert [(int(x), int(y), int(s)) for (x, y), s in zip(got["kept_xy"], got["kept_resp"])] == want["kept"], name
    _check(got, R.flat(img, excl, pattern, **p), name)


def _medium(seed=11, w=200, h=150, n_excl=40):
    return R.make_case(np.random.default_rng(seed), w, h, n_excl)


@pytest.mark.parametrize("kept_cap,all_cap", [(0, 0), (1, 1), (7, 100), (64, 65), (100000, 3)])
def test_lists_are_cut_at_their_capacities(gpu_ctx, pattern, kept_cap, all_cap):
    img, e = _medium()
    ref = R.flat(img, e, pattern, retain=100)
    assert ref["n_kept"] > 64 and ref["n_all"] > 100
    got = LC.lckf_prepare(gpu_ctx, LC.lckf_params(retain=100), img, e, want_all=True, kept_cap=kept_cap, all_cap=all_cap, fill=0xEE, raw=True)
    assert (got["n_all"], got["cut"], got["n_kept"], got["n_desc"]) == (ref["n_all"], ref["cut"], ref["n_kept"], ref["n_desc"])   # the true counts
    nk, na = min(kept_cap, ref["n_kept"]), min(all_cap, ref["n_all"])
    for f in ARRAYS:
        n = na if f.startswith("all") else nk
        assert got[f].tobytes() == ref[f][:n].tobytes(), f
        assert (got["raw"][f][n:].view(np.uint8) == 0xEE).all(), f + ": written past the list"


def _five_items():
    rng = np.random.default_rng(55)
    w, h = 100, 70
    items = [R.make_case(rng, w, h, n, kind) for n, kind in ((0, "textured"), (300, "noise"), (1, "textured"), (65, "noise"), (7, "flat"))]
    return np.stack([i[0] for i in items]), [i[1] for i in items]


def test_batch_of_5_equals_single_calls_and_specification(gpu_ctx, pattern):
    imgs, excl = _five_items()
    p = LC.lckf_params(retain=30)
    got = LC.lckf_prepare_batch(gpu_ctx, p, imgs, excl, want_all=True, fill=0xEE)
    assert len(got) == 5
    for b in range(5):
        ref = R.flat(imgs[b], excl[b], pattern, retain=30)
        _check(got[b], ref, "item %d" % b)
        _check(LC.lckf_prepare(gpu_ctx, p, imgs[b], excl[b], want_all=True), ref, "single %d" % b)
        for f in ARRAYS:
            assert (got[b]["raw"][f][len(got[b][f]):].view(np.uint8) == 0xEE).all(), (b, f)
    assert got[4]["n_all"] == 0 and got[1]["n_kept"] > 30
    assert LC.lckf_prepare_batch(gpu_ctx, p, imgs[:0], []) == []


def _per_item_scratch(w, h, kept_cap):
    """device scratch of one item as include/ov2slam_hip.h states it, every part rounded up to 256 B"""
    al = lambda v: (v + 255) // 256 * 256
    return al(4 * ((w + 31) // 32) * h) + 1024 + al((w + 63) // 64 * 64 * h) + al(16 * h) + 8 + al(8 * kept_cap)


def test_both_sides_of_the_scratch_chunk_boundary(gpu_ctx, pattern):
    imgs, excl = _five_items()
    p = LC.lckf_params(retain=30)
    per_item = _per_item_scratch(100, 70, 256)
    fits, short = (5 * per_item + 1023) // 1024, (5 * per_item - 1) // 1024
    assert short * 1024 < 5 * per_item <= fits * 1024 and short * 1024 >= 4 * per_item
    want = LC.lckf_prepare_batch(gpu_ctx, p, imgs, excl, want_all=True, kept_cap=256, all_cap=2048)
    for b in range(5):
        _check(want[b], R.flat(imgs[b], excl[b], pattern, retain=30), "item %d" % b)
    assert gpu_ctx.get_option(ov2slam_amd._lib.OV2_OPT_LCKF_SCRATCH_KB) == 256 * 1024
    for kb in (fits, short, 2 * per_item // 1024 + 1, 1):                         # one chunk; 4 + 1; 2 + 2 + 1; one item at a time
        with gpu_ctx.options(lckf_scratch_kb=kb):
            got = LC.lckf_prepare_batch(gpu_ctx, p, imgs, excl, want_all=True, kept_cap=256, all_cap=2048)
        for b in range(5):
            for f in R.FIELDS:
                assert np.asarray(got[b][f]).tobytes() == np.asarray(want[b][f]).tobytes(), (kb, b, f)
    with pytest.raises(ov2slam_amd.Ov2Error):
        gpu_ctx.set_option(ov2slam_amd._lib.OV2_OPT_LCKF_SCRATCH_KB, 0)


def test_two_runs_are_byte_identical(gpu_ctx):
    img, e = R.make_case(np.random.default_rng(3), 400, 300, 300, "noise")
    a = LC.lckf_prepare(gpu_ctx, LC.lckf_params(), img, e, want_all=True)
    b = LC.lckf_prepare(gpu_ctx, LC.lckf_params(), img, e, want_all=True)
    assert a["n_all"] > 3000
    for f in R.FIELDS:
        assert np.asarray(a[f]).tobytes() == np.asarray(b[f]).tobytes(), f


def test_custom_brief_pattern_is_honoured(gpu_ctx, pattern):
    img, e = _medium(seed=12)
    rng = np.random.default_rng(9)
    pat = rng.integers(-24, 25, (256, 4)).astype(np.int8)
    gpu_ctx.set_brief_pattern(pat)
    try:
        got = LC.lckf_prepare(gpu_ctx, LC.lckf_params(), img, e, want_all=True)
    finally:
        gpu_ctx.set_brief_pattern(None)
    _check(got, R.flat(img, e, pat), "custom pattern")
    again = LC.lckf_prepare(gpu_ctx, LC.lckf_params(), img, e, want_all=True)
    _check(again, R.flat(img, e, pattern), "built-in pattern again")
    assert got["n_desc"] > 10 and not np.array_equal(got["kept_desc"], again["kept_desc"])


def test_descriptors_equal_describe_brief_on_the_kept_points(gpu_ctx):
    img, e = _medium(seed=13, w=320, h=240)
    got = LC.lckf_prepare(gpu_ctx, LC.lckf_params(), img, e)
    d, v = ov2slam_amd.FeatureExtractor(gpu_ctx).describeBRIEF(img, got["kept_xy"].astype(np.float32))
    assert got["n_kept"] > 100 and 0 < got["n_desc"] < got["n_kept"]
    assert np.array_equal(got["kept_desc"], d) and np.array_equal(got["kept_valid"].astype(bool), v) and int(v.sum()) == got["n_desc"]


def test_tracker_form_equals_host_form(gpu_ctx, pattern):
    from ov2slam_amd import synth
    w, h = 376, 240
    prev, cur, _ = synth.frame_pair(w, h, seed=8)
    e = R.make_case(np.random.default_rng(8), w, h, 120)[1]
    vt = ov2slam_amd.VisualFrontEndTracker(gpu_ctx, w, h, use_clahe=True, fclahe_val=3.0)
    try:
        with pytest.raises(ov2slam_amd.Ov2Error):
            LC.lckf_prepare_tracker(vt, LC.lckf_params(), e)                       # no frame yet
        for img in (prev, cur):
            vt.trackFrame(img, np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), None)
            got = LC.lckf_prepare_tracker(vt, LC.lckf_params(), e, want_all=True)
            _check(got, LC.lckf_prepare(gpu_ctx, LC.lckf_params(), img, e, want_all=True), "tracker")
            _check(got, R.flat(img, e, pattern), "tracker")
    finally:
        vt.close()


def test_btracker_form(gpu_ctx, pattern):
    B, w, h = 6, 200, 150
    rng = np.random.default_rng(21)
    items = [R.make_case(rng, w, h, n) for n in (0, 40, 1, 300, 65, 7)]
    lt = ov2slam_amd.LockstepTracker(gpu_ctx, B, w, h, use_clahe=True, nbmaxkps=64)
    try:
        with pytest.raises(ov2slam_amd.Ov2Error):
            LC.lckf_prepare_btracker(lt, LC.lckf_params(), [i[1] for i in items])  # no step yet
        for b in range(B):
            lt.image_buffers[0][b][:, :w] = items[b][0]
        z = np.zeros((B, 64, 2), np.float32)
        lt.trackFrame(lt.image_buffers[0], z, z, None, np.zeros(B, np.int32))
        got = LC.lckf_prepare_btracker(lt, LC.lckf_params(retain=60), [i[1] for i in items], want_all=True)
        for b in range(B):
            _check(got[b], R.flat(items[b][0], items[b][1], pattern, retain=60), "item %d" % b)
        part = LC.lckf_prepare_btracker(lt, LC.lckf_params(retain=60), [i[1] for i in items[:2]], want_all=True)
        for b in range(2):
            _check(part[b], got[b], "prefix %d" % b)
        lt.upload(0, B)                                                         # the set holding the current frames is re-uploaded
        with pytest.raises(ov2slam_amd.Ov2Error):
            LC.lckf_prepare_btracker(lt, LC.lckf_params(), [i[1] for i in items])
    finally:
        lt.close()


def _wr(f, a):
    b = np.ascontiguousarray(a).tobytes()
    f.write(struct.pack("<q", len(b))); f.write(b)


def _rd(f, dt):
    (k,) = struct.unpack("<q", f.read(8))
    return np.frombuffer(f.read(k), dt).copy()


def test_cpp_adapter_in_both_orders(gpu_ctx, tmp_path):
    """tests/cpp/lckf_run.cpp: ov2::LoopCloser::detectAdditionalKeypoints returns the described keypoints of the Python form, in
    raster order and in the order the literal nth_element / partition (tests/cpp/lckf_order_check.cpp, no GPU) leaves them"""
    libdir = os.path.join(ROOT, "ov2slam_amd")
    run, order = tmp_path / "lckf_run", tmp_path / "lckf_order_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "lckf_run.cpp"),
                           "-o", str(run), "-L", libdir, "-lov2slam_hip", "-Wl,-rpath," + libdir])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "lckf_order_check.cpp"), "-o", str(order)])
    img, e = _medium(seed=14, w=320, h=240, n_excl=100)
    h, w = img.shape
    retain = 120
    py = LC.lckf_prepare(gpu_ctx, LC.lckf_params(retain=retain), img, e, want_all=True)
    assert py["n_all"] > retain and py["n_kept"] >= retain and 20 < py["n_desc"] < py["n_kept"]
    case, res, lists, kept = (tmp_path / n for n in ("case.bin", "res.bin", "lists.bin", "kept.bin"))
    with open(case, "wb") as f:
        _wr(f, np.array([w, h, 20, retain, 2], np.int32)); _wr(f, img); _wr(f, e)
    r = subprocess.run([str(run), str(case), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    with open(lists, "wb") as f:
        f.write(struct.pack("<iii", 1, retain, py["n_all"])); f.write(py["all_resp"].tobytes())
    subprocess.check_call([str(order), str(lists), str(kept)])
    perm = np.fromfile(kept, np.int32)[1:]                                  # indices into the all-list, the reference's order
    v = py["kept_valid"].astype(bool)
    with open(res, "rb") as f:
        for want_xy in (py["kept_xy"][v], None):
            px, resp, desc = _rd(f, np.float32).reshape(-1, 2), _rd(f, np.float32), _rd(f, np.uint8).reshape(-1, 32)
            if want_xy is None:                                             # Order::Reference
                xy = py["all_xy"][perm]
                inb = (xy[:, 0] >= 28) & (xy[:, 0] < w - 28) & (xy[:, 1] >= 28) & (xy[:, 1] < h - 28)
                want_xy = xy[inb]
                assert not np.array_equal(want_xy, py["kept_xy"][v])        # really another order
            assert np.array_equal(px, want_xy.astype(np.float32))
            look = {(int(x), int(y)): i for i, (x, y) in enumerate(py["kept_xy"])}
            idx = [look[(int(x), int(y))] for x, y in want_xy]
            assert np.array_equal(resp, py["kept_resp"][idx].astype(np.float32)) and np.array_equal(desc, py["kept_desc"][idx])
