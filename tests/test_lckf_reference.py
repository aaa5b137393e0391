"""The numpy specification of the loop closer's keyframe preparation (tests/lckf_ref.py) against itself, without a GPU: the step by
step transcription of the reference path (replay, on the oracle's cv::FAST and cv::circle) equals the order-free statement (flat) on
a generated campaign that provably reaches every situation the definition singles out; the crafted cases give their literals; the
counts of the synthetic frames are the oracle's; and the literal std::nth_element / std::partition of retainBest
(ov2slam_amd/host/loop_closer.hpp, through tests/cpp/lckf_order_check.cpp, also under the address and undefined-behaviour
sanitizers) keeps the set the histogram rule keeps."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import lckf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE_W, TILE_H = 64, 16          # any tile shape will do here: the crafted cases only need one


@pytest.fixture(scope="module")
def pattern():
    return R.builtin_pattern()


def campaign():
    """(img, excl, params): small images of every kind, exclusion lists of every size, retain on both sides of the corner count"""
    rng = np.random.default_rng(2024)
    out = []
    sizes = [(6, 9), (9, 6), (7, 7), (8, 30), (57, 57), (56, 80), (64, 64), (100, 70), (131, 97), (160, 120)]
    for i in range(48):
        w, h = sizes[i % len(sizes)]
        kind = ("textured", "noise", "textured", "flat")[i % 4] if i % 12 != 11 else "noise"
        n_excl = (0, 1, 7, 65, 300)[i % 5]
        img, e = R.make_case(rng, w, h, n_excl, kind)
        if i % 7 == 3 and n_excl:
            e[0] = (np.nan, 5.0)
        n = len(R.corners(img, 20)[0])
        retain = (300, 0, -1, max(1, n // 3), max(1, n - 1), n, 5)[i % 7]
        out.append((img, e, dict(threshold=(20, 20, 5, 40, 0, 255)[i % 6], retain=retain, radius=(2, 2, 0, 4, 7)[i % 5])))
    return out


def test_replay_equals_flat_on_the_campaign_and_the_campaign_reaches_every_event(oracle, pattern):
    seen = {}
    cases = campaign() + [(img, e, p) for _, img, e, p, _ in R.crafted_cases(TILE_W, TILE_H)]
    n_corners = 0
    for i, (img, e, p) in enumerate(cases):
        a, b = R.replay(img, e, pattern, **p), R.flat(img, e, pattern, **p)
        ok, field = R.same(a, b)
        assert ok, (i, img.shape, p, field)
        n_corners += b["n_all"]
        for ev in R.events(img, e, **p):
            seen[ev] = seen.get(ev, 0) + 1
    assert n_corners > 2000                                            # (the campaign is not made of empty images)
    missing = [ev for ev in R.EVENTS if ev not in seen]
    assert not missing, (missing, seen)


@pytest.mark.parametrize("case", R.crafted_cases(TILE_W, TILE_H), ids=lambda c: c[0])
def test_crafted_cases(oracle, pattern, case):
    name, img, excl, p, want = case
    for f in (R.flat, R.replay):
        got = f(img, excl, pattern, **p)
        assert (got["n_all"], got["cut"], got["n_kept"], got["n_desc"]) == (want["n_all"], want["cut"], want["n_kept"], want["n_desc"]), name
        assert [(int(x), int(y), int(s)) for (x, y), s in zip(got["kept_xy"], got["kept_resp"])] == want["kept"], name
        assert int(got["kept_valid"].sum()) == want["n_desc"] and not got["kept_desc"][got["kept_valid"] == 0].any()


def table_rows():
    """the three images of the counts table with their exclusion points (300 uniform points, default_rng(0)) and literals:
    corners after the suppression, after the mask, the cut score, retained, retained at the cut score, retained inside the border"""
    from ov2slam_amd import synth
    rows = [("frame_752x480", synth.frame_pair(752, 480)[0], (9251, 9159, 59, 311, 26, 239)),
            ("frame_376x240", synth.frame_pair(376, 240, seed=7)[0], (2470, 2362, 52, 303, 29, 200)),
            ("noise_752x480", np.random.default_rng(0).integers(0, 256, (480, 752), dtype=np.uint8), (35391, 35024, 137, 302, 21, 230))]
    out = []
    for name, img, lit in rows:
        h, w = img.shape
        rng = np.random.default_rng(0)
        e = np.stack([rng.uniform(0, w, 300), rng.uniform(0, h, 300)], axis=1).astype(np.float32)
        out.append((name, img, e, lit))
    return out


@pytest.mark.parametrize("row", table_rows(), ids=lambda r: r[0])
def test_counts_of_the_synthetic_frames(oracle, pattern, row):
    name, img, e, (n_nms, n_all, cut, n_kept, n_at_cut, n_desc) = row
    assert len(oracle.fast9_16(img, 20, True)[0]) == n_nms == len(R.corners(img, 20)[0])
    got = R.flat(img, e, pattern)
    assert (got["n_all"], got["cut"], got["n_kept"], int((got["kept_resp"] == cut).sum()), got["n_desc"]) == (n_all, cut, n_kept, n_at_cut, n_desc)
    if img.shape[1] < 400:
        assert R.same(got, R.replay(img, e, pattern))[0]


def test_cut_of_the_histogram_rule():
    assert R.cut_of([], 300) == (0, 1) and R.cut_of([5, 5, 5], 0) == (0, 256) and R.cut_of([5, 9], -1) == (0, 1)
    assert R.cut_of([9, 7, 7, 3], 2) == (7, 7) and R.cut_of([9, 7, 7, 3], 3) == (7, 7) and R.cut_of([9, 7, 7, 3], 1) == (9, 9)
    assert R.cut_of([9, 7, 7, 3], 4) == (0, 1) and R.cut_of([255] * 10, 9) == (255, 255) and R.cut_of([1] * 10, 3) == (1, 1)


def _order_lists(pattern):
    rng = np.random.default_rng(5)
    lists = []
    for img, e, p in campaign()[:24]:
        r = R.flat(img, e, pattern, **p)["all_resp"]
        for retain in (p["retain"], 1, 3, len(r) - 1, len(r), len(r) + 1):
            lists.append((int(retain), r))
    for n in (0, 1, 2, 3, 4, 15, 16, 17, 33, 300, 301, 1000):               # around libstdc++'s small-range thresholds; all ties
        for retain in (-1, 0, 1, 2, 3, n // 2, n - 1, n, n + 1, 300):
            lists.append((retain, np.full(n, 77, np.uint8)))
            lists.append((retain, rng.integers(1, 256, n).astype(np.uint8)))
            lists.append((retain, rng.integers(100, 104, n).astype(np.uint8)))
    return lists


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_literal_nth_element_partition_keeps_the_histogram_rules_set(tmp_path, pattern, sanitize):
    exe = tmp_path / "lckf_order_check"
    flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags +
                          [os.path.join(ROOT, "tests", "cpp", "lckf_order_check.cpp"), "-o", str(exe)])
    lists = _order_lists(pattern)
    src, dst = tmp_path / "lists.bin", tmp_path / "kept.bin"
    with open(src, "wb") as f:
        f.write(struct.pack("<i", len(lists)))
        for retain, r in lists:
            f.write(struct.pack("<ii", retain, len(r))); f.write(np.ascontiguousarray(r, np.uint8).tobytes())
    r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    raw = np.fromfile(dst, np.int32)
    o, reordered = 0, 0
    for retain, resp in lists:
        nk = int(raw[o]); got = raw[o + 1:o + 1 + nk]; o += 1 + nk
        want = R.kept_indices(resp, retain)
        assert nk == len(want) and np.array_equal(np.sort(got), want), (retain, len(resp))
        reordered += not np.array_equal(got, want)
    assert o == len(raw) and reordered > 10                                # a permutation of the set, and really not raster order
