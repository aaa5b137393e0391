"""Rows of the strip kernel k_clahe_apply_pyr (clahe.hip) on the smallest shapes where its row code can go wrong: the vertical
weights come from a per-lane table of 64 rows that stage() fills (refilled inside a taller row of cells), the fast six-row
group exists once per kind of strip (middle of the image, image edge, either), and rows are 32-bit offsets into one buffer
descriptor.  OV2_OPT_CLAHE_STRIPS 1 (strip kernel) and 2 (fused with the LUT computation) against the oracle's CLAHE + pyramid,
every level with its borders, bit for bit, batch 2.

  264 x 100, tiles 5 x 2   one strip that is both first and last
  520 x 57,  tiles 8 x 2   three strips (a middle strip exists); height no multiple of 6; a table switch inside a six-row group
  128 x 200, tiles 2 x 2   rows of cells of 100 rows, more than the table's 64: the refill
  103 x 57,  tiles 3 x 2   the instance for widths that are no multiple of 4"""
import numpy as np
import pytest

import ov2slam_amd
from ov2slam_amd import synth

pytestmark = pytest.mark.gpu

SHAPES = [((264, 100), (5, 2)), ((520, 57), (8, 2)), ((128, 200), (2, 2)), ((103, 57), (3, 2))]


@pytest.mark.parametrize("wh,tiles", SHAPES, ids=["%dx%d" % s[0] for s in SHAPES])
def test_strip_rows_equal_oracle(gpu_ctx, oracle, wh, tiles):
    w, h = wh
    rng = np.random.default_rng(5 * w + h)
    imgs = [synth.frame_pair(w, h, seed=w + 3 * h)[0], rng.integers(0, 256, (h, w), dtype=np.uint8)]
    refs = [oracle.Pyramid(oracle.clahe(im, 3.0, tiles[0], tiles[1]), 9, 3) for im in imgs]
    for force in (1, 2):
        with gpu_ctx.options(clahe_strips=force):
            P = ov2slam_amd.Pyramid(gpu_ctx, w, h, 9, 3, batch=2).build_clahe_batch(imgs, 3.0, tiles[0], tiles[1])
        for b, ref in enumerate(refs):
            assert P.levels == ref.levels
            for lvl in range(P.levels):
                g, r = P.download(lvl, b, padded=True)[0], ref.level(lvl, padded=True)[0]
                assert np.array_equal(g, r), (w, h, force, b, lvl, np.argwhere(g != r)[:4].tolist())
        P.close()
