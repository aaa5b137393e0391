"""describeBRIEF's CPU side: the numpy restatement (tests/brief_ref.py) against plain loops, the rounding the kernel uses, the
built-in pattern table, and the recovery of a pattern from probe descriptors (tools/brief_pattern_from_probes.py)."""
import importlib.util
import os
import re

import numpy as np
import pytest

from tests import brief_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _builtin_pattern():
    txt = open(os.path.join(ROOT, "ov2slam_amd", "csrc", "brief_pattern.hpp")).read()
    body = txt[txt.index("= {") + 3:txt.index("};")]
    return np.array([int(v) for v in re.findall(r"-?\d+", body)], np.int8).reshape(256, 4)


def _edge_points(w, h, rng, n_rand=20):
    pts = [rng.uniform(-5, w + 5, n_rand), rng.uniform(-5, h + 5, n_rand)]
    pts = list(np.stack(pts, 1))
    for v in np.arange(27.0, 29.01, 0.25):
        pts += [(v, h / 2), (w / 2, v), (w - 57.0 + v, h / 2), (w / 2, h - 57.0 + v)]
    pts += [(27.5, 27.5), (28.5, 28.5), (w - 28.5, h - 28.5), (w - 29.5, h - 29.5), (w - 28.5, 40.0), (40.0, h - 28.5),
            (np.nan, 40.0), (40.0, np.inf), (-30.0, 40.0), (40.5, 40.5), (40.5, 40.5)]
    return np.array(pts, np.float32)


@pytest.mark.parametrize("w,h,seed", [(57, 57, 1), (58, 61, 2), (61, 59, 3), (75, 66, 4)])
def test_restatement_matches_scalar_loops(w, h, seed):
    """bit order (MSB first), the border rule with its .5 ties, the odd-size corner case (in-image pixels only)"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    pts = _edge_points(w, h, rng)
    pat = rng.integers(-24, 25, (256, 4)).astype(np.int8)
    pat[:8] = [[24, 24, -24, -24], [-24, -24, 24, 24], [0, 24, 0, -24], [24, 0, -24, 0], [3, 3, 3, 3], [0, 0, 1, 0], [-24, 24, 24, -24], [0, 0, 0, 0]]
    d1, v1 = R.describe(img, pts, pat)
    d2, v2 = R.describe_scalar(img, pts, pat)
    assert np.array_equal(v1, v2)
    assert np.array_equal(d1, d2)
    assert not d1[~v1].any()
    if w > 56 and h > 56:
        assert v1.sum() > 10


def test_restatement_bit_order_and_border_rule_by_hand():
    img = np.zeros((60, 60), np.uint8)
    img[30, 36] = 200                       # inside box(0, +6) around (30, 30) only
    pat = np.zeros((256, 4), np.int8)
    pat[0] = (0, 0, 0, 6)                   # S(0,0) = 0 < S(0,6) = 200: the MSB of byte 0
    pat[9] = (0, 0, 0, 6)                   # test 9: byte 1, bit 6
    pat[10] = (0, 6, 0, 0)                  # 200 < 0: no
    d, v = R.describe(img, np.array([[30.0, 30.0]], np.float32), pat)
    assert v.tolist() == [True]
    assert d[0, 0] == 0x80 and d[0, 1] == 0x40 and not d[0, 2:].any()
    # 28 <= rint(x) < 60 - 28 = 32: 27.5 -> 28 (in), 31.5 -> 32 (out), 30.5 -> 30 (in), 32.49 -> 32 (out), 27.49 -> 27 (out)
    xs = np.array([27.5, 31.5, 30.5, 32.49, 27.49, 31.4999], np.float32)
    v = R.border_valid(np.stack([xs, np.full_like(xs, 30)], 1), 60, 60)
    assert v.tolist() == [True, False, True, False, False, True]
    assert not R.border_valid(np.array([[28, 28]], np.float32), 56, 200).any()      # W <= 56: nothing survives


def test_kernel_rounding_exhaustive():
    """Every float32 in [27.5, 4096): the kernel's floorf(x + 0.5f) (float arithmetic) is OpenCV's (int)((double)x + 0.5), and its
    rintf border test is saturate_cast's round-half-to-even.  Also: a survivor's centre is rint(x) or rint(x) + 1, the latter only
    on an exact .5 -- the one way a box can pass the image edge (rule 5)."""
    lo = np.float32(27.5).view(np.uint32)
    hi = np.float32(4096.0).view(np.uint32)
    step = 1 << 23
    for a in range(int(lo), int(hi), step):
        x = np.arange(a, min(a + step, int(hi)), dtype=np.uint32).view(np.float32)
        k = np.floor(x + np.float32(0.5))
        assert k.dtype == np.float32
        xd = x.astype(np.float64)
        ref = np.trunc(xd + 0.5)
        assert np.array_equal(k.astype(np.float64), ref)
        fl = np.floor(xd)
        frac = xd - fl
        even = np.where(frac < 0.5, fl, np.where(frac > 0.5, fl + 1, np.where(fl % 2 == 0, fl, fl + 1)))
        r = np.rint(x)
        assert np.array_equal(r.astype(np.float64), even)
        up = ref != even
        assert np.all(ref[up] == even[up] + 1) and np.all(frac[up] == 0.5)


def test_builtin_pattern_is_the_generator_output():
    gen = _tool("gen_brief_pattern")
    txt = open(os.path.join(ROOT, "ov2slam_amd", "csrc", "brief_pattern.hpp")).read()
    assert txt == gen.render(gen.generate())
    p = _builtin_pattern()
    assert np.array_equal(p, np.array(gen.generate(), np.int8))
    assert p.min() >= -24 and p.max() <= 24 and p.min() == -24 and p.max() == 24
    assert not np.all(p[:, :2] == p[:, 2:], axis=1).any()


def test_probe_recovery_roundtrip():
    """a random pattern (offsets covering +-24, some a == b pairs) -> numpy describe of the probe set -> the recovered table"""
    probe = _tool("brief_probe")
    rec = _tool("brief_pattern_from_probes")
    rng = np.random.default_rng(11)
    pat = rng.integers(-24, 25, (256, 4)).astype(np.int8)
    pat[0] = (24, 24, -24, -24); pat[1] = (-24, 24, 24, -24); pat[2] = (0, 0, 0, 1); pat[3] = (5, -7, 5, -7)
    pat[4] = (10, 3, 10, 3); pat[5] = (-24, -24, -24, -23); pat[6] = (3, 24, 2, 24); pat[7] = (0, 0, 8, 8); pat[8] = (0, 0, 9, 0)
    degenerate = np.all(pat[:, :2] == pat[:, 2:], axis=1)
    assert degenerate.sum() >= 2
    bright, dark = probe.probe_images()
    kp = probe.probe_keypoints()
    db, vb = R.describe_stack(bright, kp, pat)
    dd, vd = R.describe_stack(dark, kp, pat)
    assert vb.all() and vd.all()
    got = rec.recover(db[:, 0], dd[:, 0])
    want = pat.copy()
    want[degenerate] = 0
    assert np.array_equal(got, want)


def test_opencv_capture():
    """The restatement with OpenCV's recovered table against descriptors OpenCV itself computed (captured elsewhere)."""
    gold = os.path.join(ROOT, "tests", "golden")
    pat_f = os.path.join(gold, "brief_pattern_opencv.npy")
    if not os.path.exists(pat_f):
        pytest.skip("no OpenCV BRIEF capture: on a host with OpenCV + contrib run  python tools/brief_probe.py /tmp/brief_in && "
                    "cmake -S tools/ref_capture -B /tmp/ref_capture && cmake --build /tmp/ref_capture --target ov2_capture_brief && "
                    "mkdir -p /tmp/brief_out && /tmp/ref_capture/ov2_capture_brief /tmp/brief_in /tmp/brief_out && "
                    "python tools/brief_pattern_from_probes.py /tmp/brief_out")
    pat = np.load(pat_f)
    assert pat.shape == (256, 4) and np.abs(pat).max() <= 24
    probe = _tool("brief_probe")
    for name, imgs, kps in probe.frame_sets():
        want_d = np.load(os.path.join(gold, "brief_opencv", name + ".desc.npy"))
        want_v = np.load(os.path.join(gold, "brief_opencv", name + ".valid.npy")).astype(bool)
        w = imgs.shape[2]
        corner = (np.float32(kps[:, 0]) == w - 28.5) if w % 2 else np.zeros(len(kps), bool)
        for i, img in enumerate(imgs):
            d, v = R.describe(img, kps, pat)
            assert np.array_equal(v, want_v[i]), name
            keep = ~corner                     # rule 5: OpenCV reads past its integral image there
            assert np.array_equal(d[keep], want_d[i][keep]), name


def test_product_does_not_import_the_restatement():
    for dp, _, files in os.walk(os.path.join(ROOT, "ov2slam_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp")):
                assert not re.search(r"\bbrief_ref\b", open(os.path.join(dp, f), errors="replace").read()), f
