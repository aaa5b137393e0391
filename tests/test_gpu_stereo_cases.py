"""ov2_stereo_match / ov2_stereo_match_batch / ov2_line_min_sad (csrc/stereo.hip, the stereo mode of k_track_klt in lk.hip and of
k_track_klt_w in lkw.hip) against oracle.stereo_matching and oracle.line_min_sad on the scenes of tests/stereo_cases.py, whose
branch population tests/test_stereo_cases.py asserts on the oracle alone.  Everything bit for bit: stereo_ok as booleans, right_px as
raw float32 bits.  Both tracking kernels, every window instance of the row kernel, both accumulator modes, rectified and
non-rectified with distortion, a fisheye pair (status left out within 1e-3 px of the gate: stereo_cases.near_gate), partial wavefronts / work-groups, every nklt_pyr_lvl, and the batch form."""
import numpy as np
import pytest

import ov2slam_amd
from ov2slam_amd import stereo
from ov2slam_amd import _lib as L

from tests import stereo_cases as SC

pytestmark = pytest.mark.gpu

TRACK_IMPL = {"wave": L.OV2_TRACK_IMPL_WAVE, "row": L.OV2_TRACK_IMPL_ROW}
LK_IMPL = {"row": L.OV2_LK_IMPL_ROW, "lane3": L.OV2_LK_IMPL_LANE3}
# OV2_OPT_TRACK_IMPL chooses between two kernels for window 9 only; every other window has the row kernel alone: one run
FUSED = [(name, win, impl) for name, win in SC.CASE_WINS for impl in (("wave", "row") if win == 9 else ("row",))]
SEQUENCE = [(name, win, impl) for name, win in SC.CASE_WINS for impl in ("row", "lane3")]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what, near_gate=None):
    """near_gate: the key points whose status is left out (stereo_cases.near_gate: the fisheye case alone); positions always count"""
    ok, right = got
    rok, rright = want
    assert ok.shape == rok.shape and right.shape == rright.shape, what
    status = (ok != rok) if near_gate is None else (ok != rok) & ~near_gate
    bad = np.nonzero(status | (_bits(right) != _bits(rright)).any(axis=-1))[0]
    assert len(bad) == 0, "%s: %d of %d keypoints differ, first %d: ok %s / %s, right %s / %s" % (
        what, len(bad), len(ok), bad[0], ok[bad[0]], rok[bad[0]], right[bad[0]], rright[bad[0]])


class _Rig:
    """the device side of the cases: pyramids (built once per module), calibrations, one FeatureTracker"""

    def __init__(self, ctx):
        self.ctx, self.trk, self._pyrs = ctx, ov2slam_amd.FeatureTracker(ctx, 30, 0.01), {}

    def pyrs(self, c):
        key = id(c)
        if key not in self._pyrs:
            self._pyrs[key] = tuple(ov2slam_amd.Pyramid(self.ctx, c["w"], c["h"], c["win"], SC.MAX_LEVEL).build(c[k]) for k in ("left", "right"))
        return self._pyrs[key]

    def cal(self, c):
        return ov2slam_amd.CameraCalibration(self.ctx, c["model"], *c["K"], D=c["D"])

    def run(self, fn, c, n=None, nklt_pyr_lvl=None):
        n = len(c["kps"]) if n is None else n
        pl, pr = self.pyrs(c)
        return fn(self.trk, pl, pr, c["kps"][:n], c["kps_unpx"][:n], self.cal(c), rect=c["rect"], Frl=c["Frl"], nklt_win_size=c["win"],
                  nklt_pyr_lvl=c["nklt_pyr_lvl"] if nklt_pyr_lvl is None else nklt_pyr_lvl, priors3d=SC.prefix_priors(c, n))

    def close(self):
        for pl, pr in self._pyrs.values():
            pl.close(); pr.close()
        self._pyrs = {}


@pytest.fixture(scope="module")
def rig(gpu_ctx):
    r = _Rig(gpu_ctx)
    yield r
    r.close()


@pytest.mark.parametrize("name,win,impl", FUSED)
def test_fused_form_against_the_oracle(gpu_ctx, oracle, rig, name, win, impl):
    c = SC.case(name, win)
    with gpu_ctx.options(track_impl=TRACK_IMPL[impl]):
        got = rig.run(stereo.stereo_matching_fused, c)
    _same(got, (c["ok"], c["right_px"]), "%s win %d %s" % (name, win, impl), c["near_gate"])
    assert 2 * got[0].sum() >= len(got[0])


@pytest.mark.parametrize("name,win,impl", SEQUENCE)
def test_call_sequence_against_the_oracle(gpu_ctx, oracle, rig, name, win, impl):
    c = SC.case(name, win)
    with gpu_ctx.options(lk_impl=LK_IMPL[impl]):
        got = rig.run(stereo.stereo_matching, c)
    _same(got, (c["ok"], c["right_px"]), "%s win %d %s" % (name, win, impl), c["near_gate"])


@pytest.mark.parametrize("name,impl", [("euroc_half", "wave"), ("euroc_half", "row"), ("odd_w7", "row"), ("odd_w11_unrect", "row")])
def test_float_accumulators_in_stereo_mode(gpu_ctx, oracle, rig, name, impl):
    """k_track_klt_w<true> (window 9, wave) and k_track_klt<W, true> with the SAD priors applied inside the kernel, against the oracle
    in LK_ACC_FLOAT_UI4; on contrast-stretched images, where float sums round: the result is not the INT64 mode's"""
    c = SC.case(name, contrast=True)
    want = SC.oracle_run(c, float_acc=True)
    with gpu_ctx.options(track_impl=TRACK_IMPL[impl]):
        int_ok, int_right = rig.run(stereo.stereo_matching_fused, c)
        with gpu_ctx.options(lk_acc=L.OV2_LK_ACC_FLOAT_UI4):
            got = rig.run(stereo.stereo_matching_fused, c)
        assert gpu_ctx.get_option(L.OV2_OPT_LK_ACC) == L.OV2_LK_ACC_INT64
    _same(got, want, "%s %s float accumulators" % (name, impl))
    _same((int_ok, int_right), (c["ok"], c["right_px"]), "%s %s int64 on the stretched images" % (name, impl))
    both = got[0] & int_ok
    n_diff = int((_bits(got[1][both]) != _bits(int_right[both])).any(axis=1).sum())
    assert n_diff > 0, "the float mode returned the INT64 mode's bits everywhere: it did not run"
    assert gpu_ctx.get_option(L.OV2_OPT_LK_ACC) == L.OV2_LK_ACC_INT64


@pytest.mark.parametrize("n", [0, 1, 2, 3, 5, 63, 64, 65])
def test_prefixes_partial_groups(gpu_ctx, oracle, rig, n):
    """k_line_min_sad handles 4 keypoints per work-group, k_track_klt 4 per wavefront: the first n keypoints of euroc_half"""
    c = SC.case("euroc_half")
    want = SC.oracle_run(c, n=n)
    assert want[0].shape == (n,) and want[1].shape == (n, 2)
    for impl in ("wave", "row"):
        with gpu_ctx.options(track_impl=TRACK_IMPL[impl]):
            got = rig.run(stereo.stereo_matching_fused, c, n=n)
        assert got[0].dtype == bool and got[1].dtype == np.float32
        _same(got, want, "first %d keypoints, %s" % (n, impl))


@pytest.mark.parametrize("lvl", [0, 1, 2, 3])
def test_every_nklt_pyr_lvl(gpu_ctx, oracle, rig, lvl):
    """the SAD level, `up` and the depth of the full-pyramid pass follow nklt_pyr_lvl; the one-level pass stays at 1"""
    c = SC.case("flat_strip")
    want = SC.oracle_run(c, nklt_pyr_lvl=lvl)
    for impl in ("wave", "row"):
        with gpu_ctx.options(track_impl=TRACK_IMPL[impl]):
            _same(rig.run(stereo.stereo_matching_fused, c, nklt_pyr_lvl=lvl), want, "fused, level %d, %s" % (lvl, impl))
    _same(rig.run(stereo.stereo_matching, c, nklt_pyr_lvl=lvl), want, "call sequence, level %d" % lvl)
    if lvl != c["nklt_pyr_lvl"]:
        assert not np.array_equal(_bits(want[1]), _bits(c["right_px"]))


@pytest.mark.parametrize("name,lvl", [("flat_strip", 3), ("flat_strip", 0), ("odd_w7", 2)])
def test_line_min_sad_at_the_borders(gpu_ctx, oracle, rig, name, lvl):
    """getLineMinSAD alone: 400 points within 6 px of the borders of the level (corners, last row and column included), 200 inside;
    on level 0 going right also points whose running `c += 1` crosses 4 .. 128 (the float sum rounds there).  tests/test_stereo_cases.py
    asserts that these sets hold "nothing found" and grown half windows."""
    c = SC.case(name)
    pl, pr = rig.pyrs(c)
    il, ir = c["opl"].level(lvl)[0], c["opr"].level(lvl)[0]
    lh, lw = il.shape
    assert pl.level_size(lvl) == (lw, lh)
    pts = SC.sad_points(lw, lh, np.random.default_rng(lvl), pow2_right=(lvl == 0))
    for win in (3, 5, 7, 9):
        for go_left in (True, False):
            xp, err = rig.trk.getLineMinSAD(pl, pr, lvl, pts, win, go_left)
            rxp, rerr = oracle.line_min_sad(il, ir, pts, win, go_left)
            bad = np.nonzero((_bits(xp) != _bits(rxp)) | (_bits(err) != _bits(rerr)))[0]
            assert len(bad) == 0, "win %d %s: %d points differ, first %s: %s %s / %s %s" % (
                win, "left" if go_left else "right", len(bad), pts[bad[0]], xp[bad[0]], err[bad[0]], rxp[bad[0]], rerr[bad[0]])
            assert (rxp == -1).any() and (rxp != -1).sum() > 300


@pytest.mark.parametrize("name", ["euroc_half", "euroc_half_unrect"])
def test_batch_form_against_the_oracle(gpu_ctx, oracle, name):
    """ov2_stereo_match_batch on four items of five-item pyramids (n_items < batch), counts [130, 0, 1, 67] in 150 slots: per item the
    oracle's result on that item; slots beyond the count and the fifth item stay zero"""
    batch, n_items, n_max, counts = 5, 4, 150, [130, 0, 1, 67]
    items = [SC.case(name, seed=s) for s in (616, 11, 12, 13)]
    w, h = items[0]["w"], items[0]["h"]
    lefts = np.stack([c["left"] for c in items] + [items[1]["right"]])
    rights = np.stack([c["right"] for c in items] + [items[2]["left"]])
    plb = ov2slam_amd.Pyramid(gpu_ctx, w, h, 9, SC.MAX_LEVEL, batch=batch).build(lefts)
    prb = ov2slam_amd.Pyramid(gpu_ctx, w, h, 9, SC.MAX_LEVEL, batch=batch).build(rights)
    trk = ov2slam_amd.FeatureTracker(gpu_ctx, 30, 0.01)
    c0 = items[0]
    cal = ov2slam_amd.CameraCalibration(gpu_ctx, "pinhole", *c0["K"], D=c0["D"])
    # unused slots hold NaN: nothing may read them
    K = np.full((batch, n_max, 2), np.nan, np.float32); U = K.copy(); P = K.copy(); H = np.ones((batch, n_max), np.uint8)
    for b, (c, n) in enumerate(zip(items, counts)):
        K[b, :n] = c["kps"][:n]; U[b, :n] = c["kps_unpx"][:n]; P[b, :n] = c["kps"][:n]; H[b, :n] = 0
        for i, p in SC.prefix_priors(c, n).items():
            P[b, i] = p; H[b, i] = 1
    try:
        for impl in ("wave", "row"):
            with gpu_ctx.options(track_impl=TRACK_IMPL[impl]):
                ok, right = stereo.stereo_match_batch_arrays(trk, plb, prb, n_items, n_max, K, U, P, H, np.array(counts, np.int32), cal,
                                                             rect=c0["rect"], Frl=c0["Frl"])
            assert ok.shape == (batch, n_max) and right.shape == (batch, n_max, 2)
            for b, (c, n) in enumerate(zip(items, counts)):
                _same((ok[b, :n], right[b, :n]), SC.oracle_run(c, n=n), "%s item %d, %s" % (name, b, impl))
                assert not ok[b, n:].any() and not _bits(right[b, n:]).any()
            assert not ok[n_items:].any() and not _bits(right[n_items:]).any()
            assert ok[0].sum() >= 65 and ok[3].sum() >= 30
    finally:
        plb.close(); prb.close()
