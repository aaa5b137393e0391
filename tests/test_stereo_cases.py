"""The scenes of tests/stereo_cases.py on the CPU oracle alone: every branch that tests/test_gpu_stereo_cases.py means to compare is
populated.  These are conditions on the cases, not measurements of the code: a seed that misses one is changed, never the condition."""
import numpy as np
import pytest

from tests import stereo_cases as SC


@pytest.mark.parametrize("name,win", SC.CASE_WINS)
def test_case_populates_the_branches(oracle, capsys, name, win):
    c = SC.case(name, win)
    s, k = SC.stages(c), SC.counts(c)
    with capsys.disabled():
        print("\n  %s, window %d, nklt_pyr_lvl %d, %s: %s" % (name, win, c["nklt_pyr_lvl"], "rectified" if c["rect"] else "non-rectified",
                                                             ", ".join("%s %s" % kv for kv in k.items())))
    n, w, h = k["n"], c["w"], c["h"]
    assert c["kps"].dtype == np.float32 and c["kps"][:, 0].min() >= 0 and c["kps"][:, 0].max() <= w - 1
    assert c["kps"][:, 1].min() >= 0 and c["kps"][:, 1].max() <= h - 1
    assert c["nklt_pyr_lvl"] <= c["opl"].levels - 1
    # the stages restated from the oracle's entry points are the flow oracle.stereo_matching runs
    assert np.array_equal(s["tracked"], (c["right_px"] != 0).any(axis=1))
    assert not (c["ok"] & ~s["tracked"]).any()
    if c["rect"]:
        assert k["sad_none"] >= 3                                             # SAD "nothing found"
    if name in ("euroc_half", "flat_strip"):                                  # half-window spread
        hw = set(k["halfwin"])
        assert {0, 1, 2, 3} <= hw and max(hw) >= 4, hw
    assert k["retried"] >= 5 and 2 * k["first_ok"] >= k["with_3d"]            # retries
    if c["nklt_pyr_lvl"] >= 2:      # (at nklt_pyr_lvl 1 the retry has the depth of the pass that failed: both starts can end alike)
        assert k["retry_distinct"] >= 1                                        # a retry from the 3-D prior itself would show
    assert k["gate_rejected"] >= 10 and 2 * k["ok"] >= n                      # gate
    assert k["untracked"] >= 3                                                # no track
    # the status of at most 2 % of the points is left out of the device comparison, and under the pinhole model of none
    assert c["near_gate"].sum() <= (0.02 * n if c["model"] == "fisheye" else 0)
    if name == "fisheye_unrect":
        assert c["model"] == "fisheye" and not c["rect"] and np.array_equal(c["Frl"], SC.F_XTRANS) and c["nklt_pyr_lvl"] == 1
        pin = oracle.compute_keypoints(oracle.CAM_PINHOLE, c["K"], c["D"], np.eye(3), c["kps"])[0]
        assert np.abs(c["kps_unpx"] - pin).max() > 0.05                       # the fisheye undistortion, not the pinhole one


def test_half_window_quirk(oracle):
    """half_window() against the oracle's getLineMinSAD on a flat image pair: the oracle returns -1 exactly where the half window
    ends <= 0; the grown windows (up to 10 for window 9: SAD_MAX_WS 21 in stereo.hip) are reached"""
    lw, lh = 33, 13
    img = np.full((lh, lw), 77, np.uint8)
    pts = SC.sad_points(lw, lh, np.random.default_rng(1))
    for win in (3, 5, 7, 9):
        hw = SC.half_windows(pts, lw, lh, win)
        xp, err = oracle.line_min_sad(img, img, pts, win, True)
        scanned = pts[:, 0] >= hw                                             # the leftward scan has at least its first candidate
        assert np.array_equal(xp == -1, ~((hw > 0) & scanned))
        # x + h0 >= w adds at most h0 - 2, then y + h >= rows at most h - 2 again: growth needs h0 >= 3 (windows 7 and 9)
        h0 = win // 2
        assert hw.max() == max(h0, 4 * h0 - 6)
    assert SC.half_windows(np.array([[lw - 1, lh - 1]], np.float32), lw, lh, 9)[0] == 10


def test_sad_point_sets(oracle):
    """the point sets of the getLineMinSAD comparison contain "nothing found" and grown half windows on every level they are used on"""
    for name, lvl in (("flat_strip", 3), ("flat_strip", 0), ("odd_w7", 2)):
        c = SC.case(name)
        il, ir = c["opl"].level(lvl)[0], c["opr"].level(lvl)[0]
        lh, lw = il.shape
        pts = SC.sad_points(lw, lh, np.random.default_rng(lvl), pow2_right=(lvl == 0))
        assert len(pts) >= 600 and pts[:, 0].min() == 0 and pts[:, 0].max() == lw - 1 and pts[:, 1].max() == lh - 1
        for win in (3, 5, 7, 9):
            hw = SC.half_windows(pts, lw, lh, win)
            for go_left in (True, False):
                xp, _ = oracle.line_min_sad(il, ir, pts, win, go_left)
                assert (xp == -1).any(), (name, lvl, win, go_left)
                if win >= 7:                                                  # (windows 3 and 5 cannot grow: test_half_window_quirk)
                    assert ((xp != -1) & (hw > win // 2)).any(), (name, lvl, win, go_left)
                else:
                    assert ((xp != -1) & (hw < win // 2)).any() or win == 3, (name, lvl, win, go_left)


@pytest.mark.parametrize("name", ["euroc_half", "odd_w7", "odd_w11_unrect"])
def test_float_accumulators_change_the_result(oracle, capsys, name):
    """on the contrast-stretched images the float-accumulator order of an x86 OpenCV 4.x build returns other bits than the exact
    integer sums: a device run in that mode that equals the oracle's cannot have been the INT64 kernel"""
    c = SC.case(name, contrast=True)
    ok_i, right_i = c["ok"], c["right_px"]
    ok_f, right_f = SC.oracle_run(c, float_acc=True)
    both = ok_i & ok_f
    n_diff = int((right_i[both].view(np.uint32) != right_f[both].view(np.uint32)).any(axis=1).sum())
    with capsys.disabled():
        print("\n  %s, contrast-stretched: %d of %d positions differ between the accumulator modes, %d status flips"
              % (name, n_diff, both.sum(), (ok_i != ok_f).sum()))
    assert n_diff > 0 and 2 * both.sum() >= len(ok_i)
    assert oracle.lib().orc_get_lk_acc_mode() == oracle.LK_ACC_INT64


def test_prefixes_and_levels_differ(oracle):
    """the prefix runs and the nklt_pyr_lvl runs are runs of their own: shapes follow n, and another level gives other positions"""
    c = SC.case("euroc_half")
    for n in (0, 1, 5, 65):
        ok, right = SC.oracle_run(c, n=n)
        assert ok.shape == (n,) and right.shape == (n, 2)
        assert np.array_equal(ok, c["ok"][:n])                                # keypoints are independent of each other
    f = SC.case("flat_strip")
    rights = [SC.oracle_run(f, nklt_pyr_lvl=l)[1] for l in range(4)]
    for l in range(3):
        assert not np.array_equal(rights[l], rights[3])


def test_cases_are_cached_and_distinct():
    a, b = SC.case("euroc_half"), SC.case("euroc_half")
    assert a is b
    d = SC.case("euroc_half", seed=7)
    assert not np.array_equal(a["left"], d["left"]) and not np.array_equal(a["kps"], d["kps"])
    u = SC.case("euroc_half_unrect")
    assert np.array_equal(a["kps"], u["kps"]) and not np.array_equal(a["kps_unpx"], u["kps_unpx"]) and u["Frl"] is not None
