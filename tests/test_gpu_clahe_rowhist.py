"""The row form of the fused strip kernel's histograms (clahe.hip: clahe_lut_row_hist; chosen by clahe_plan.hpp): whole image rows,
12 bytes per lane, into 16-bit counters with two tiles per dword.  Each case runs a batch of 3 different images with the fused
kernel forced (OV2_OPT_CLAHE_STRIPS = 2) and compares every padded pyramid level of every item, bit for bit, with the oracle
(CLAHE, then the pyramid) and with forms 1 and 0, which keep the per-tile histogram code.  Counts are integers: no tolerance.

The geometries are the smallest at which the lane-to-tile mapping can go wrong (tests/test_clahe_plan.py pins which of them the
plan gives the row form):
  64 x 8 / 2 x 1      the least the strip kernel takes, no padding (LK window 3 and two levels: a 9-pixel border would mirror
                      an 8-row image twice);
  103 x 57 / 3 x 2    tile edges inside dwords, padding right and below, an odd tile count (one half-used pair block);
  264 x 100 / 5 x 2, 376 x 240 / 7 x 4;
  256 x 64 / 16 x 2   16 tiles of 16 pixels -- its eight pair blocks beside ONE strip would cost a resident work-group, so the plan
                      keeps the tile form; 240 x 64 / 15 x 2 is the same layout with eight blocks (the last half used) in the row form;
  200 x 60 / 4 x 4    th = 15: a row of tiles shorter than the four rows in flight per lane and wavefront;
  1024 x 64 / 8 x 2   more than 192 dwords per row: the chunk loop;
  752 x 480 / 15 x 9  EuRoC;
  1241 x 376 / 24 x 7 refused by the plan (three LUT wavefronts): the fallback."""
import numpy as np
import pytest

import ov2slam_amd
from ov2slam_amd import synth

pytestmark = pytest.mark.gpu


def _check(gpu_ctx, oracle, imgs, tiles):
    h, w = imgs[0].shape
    win, max_level = (9, 3) if h >= 24 else (3, 1)
    refs = [oracle.Pyramid(oracle.clahe(im, 3.0, tiles[0], tiles[1]), win, max_level) for im in imgs]
    for force in (2, 1, 0):
        with gpu_ctx.options(clahe_strips=force):
            P = ov2slam_amd.Pyramid(gpu_ctx, w, h, win, max_level, batch=len(imgs)).build_clahe_batch(imgs, 3.0, tiles[0], tiles[1])
        assert P.levels == refs[0].levels
        for b, ref in enumerate(refs):
            for lvl in range(P.levels):
                got, want = P.download(lvl, b=b, padded=True)[0], ref.level(lvl, padded=True)[0]
                assert np.array_equal(got, want), (w, h, tiles, force, b, lvl, np.argwhere(got != want)[:4].tolist())
        P.close()


@pytest.mark.parametrize("wh,tiles", [((64, 8), (2, 1)), ((103, 57), (3, 2)), ((264, 100), (5, 2)), ((376, 240), (7, 4)),
                                       ((256, 64), (16, 2)), ((240, 64), (15, 2)), ((200, 60), (4, 4)), ((1024, 64), (8, 2)),
                                       ((752, 480), (15, 9)), ((1241, 376), (24, 7))])
def test_row_histogram_equals_oracle_and_tile_forms(gpu_ctx, oracle, wh, tiles):
    w, h = wh
    rng = np.random.default_rng(3 * w + h)
    imgs = [synth.frame_pair(w, h, seed=w + h)[0], rng.integers(0, 256, (h, w), dtype=np.uint8),
            np.clip(synth.frame_pair(w, h, seed=w + h + 1)[0].astype(np.int32) // 3 + rng.integers(0, 30, (h, w)), 0, 255).astype(np.uint8)]
    _check(gpu_ctx, oracle, imgs, tiles)


@pytest.mark.parametrize("wh,tiles", [((752, 480), (15, 9)), ((103, 57), (3, 2))])
def test_row_histogram_low_entropy_frames(gpu_ctx, oracle, wh, tiles):
    """Every lane of a ds_add on a handful of counters: constant 128, all 255 (the top bin of both halves of a dword), and 80 % of the
    pixels on 8 grey levels."""
    w, h = wh
    rng = np.random.default_rng(7 * w + h)
    base = synth.frame_pair(w, h, seed=w + 11 * h)[0].astype(np.int32)
    sel = rng.uniform(size=base.shape) < 0.8
    imgs = [np.full((h, w), 128, np.uint8), np.full((h, w), 255, np.uint8), np.where(sel, base // 32, base // 4).astype(np.uint8)]
    _check(gpu_ctx, oracle, imgs, tiles)
