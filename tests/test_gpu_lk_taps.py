"""k_fb_klt3 (lk3.hip) with both template-build instances in one wavefront: 2 items of 160 x 120, 4 pyramid levels, 40 keypoints
per item of which 12 lie within 9 pixels of an image edge -- their windows overlap the border, so a wavefront builds its templates
with the border masks at the levels where one of its keypoints needs them (for all its lanes) and without them elsewhere.  The
derivative taps carry their rounding
constant in a scalar register and the first product of every sum starts it (three-address v_dot2_i32_i16); positions (as bits)
and status must equal the oracle's forward-backward tracker, with 1 and with 3 pyramid levels."""
import ctypes as C

import numpy as np
import pytest

import ov2slam_amd
from ov2slam_amd import synth
from ov2slam_amd.loop_closer import _DeviceArrays

pytestmark = pytest.mark.gpu

W, H, B, N, N_EDGE = 160, 120, 2, 40, 12


@pytest.fixture(scope="module")
def scene():
    rng = np.random.default_rng(23)
    prevs, curs = [], []
    kps, pri = np.zeros((B, N, 2), np.float32), np.zeros((B, N, 2), np.float32)
    for b in range(B):
        p, c, flow = synth.frame_pair(W, H, seed=31 + b, shift=(1.1 + 0.4 * b, -0.7), theta=0.002 * (b + 1))
        prevs.append(p); curs.append(c)
        inner = np.stack([rng.uniform(12, W - 13, N - N_EDGE), rng.uniform(12, H - 13, N - N_EDGE)], 1)
        t = rng.uniform(0, 8.5, N_EDGE)                                    # distance to the edge: within 9 pixels
        along_x, along_y = rng.uniform(0, W - 1, N_EDGE), rng.uniform(0, H - 1, N_EDGE)
        side = np.arange(N_EDGE) % 4                                       # left, right, top, bottom: 3 each
        edge = np.stack([np.where(side == 0, t, np.where(side == 1, W - 1 - t, along_x)),
                         np.where(side == 2, t, np.where(side == 3, H - 1 - t, along_y))], 1)
        k = np.concatenate([inner, edge]).astype(np.float32)
        d = np.minimum(np.minimum(k[:, 0], W - 1 - k[:, 0]), np.minimum(k[:, 1], H - 1 - k[:, 1]))
        assert int((d < 9).sum()) == N_EDGE
        k = k[rng.permutation(N)]                                          # edge and inner keypoints share wavefronts
        kps[b] = k
        pri[b] = (flow(k) + rng.normal(0, 0.8, k.shape)).astype(np.float32)
    return prevs, curs, kps, pri


@pytest.mark.parametrize("nbpyrlvl", [1, 3])
def test_fb_klt_taps_equal_oracle(gpu_ctx, oracle, scene, nbpyrlvl):
    prevs, curs, kps, pri = scene
    Pp = ov2slam_amd.Pyramid(gpu_ctx, W, H, 9, 3, batch=B).build(np.stack(prevs))
    Pc = ov2slam_amd.Pyramid(gpu_ctx, W, H, 9, 3, batch=B).build(np.stack(curs))
    assert Pp.levels == 4
    dev = _DeviceArrays()
    try:
        dk, dp = dev.upload(kps), dev.upload(pri)
        ds, dt = dev.upload(np.full((B, N), 7, np.uint8)), dev.upload(np.zeros(2, np.int64))
        gpu_ctx.sync()
        with gpu_ctx.options(lk_impl=ov2slam_amd._lib.OV2_LK_IMPL_LANE3):
            ov2slam_amd._lib.check(gpu_ctx.lib.ov2_fb_klt_d(gpu_ctx.h, Pp.h_pyr, Pc.h_pyr, 9, nbpyrlvl, 30, 0.01, 30.0, 0.5, C.c_void_p(dk), C.c_void_p(dp), N,
                                                            None, C.c_void_p(ds), C.c_void_p(dt)))
        gpu_ctx.sync()
        gp, gs = dev.download(dp, np.empty((B, N, 2), np.float32)), dev.download(ds, np.empty((B, N), np.uint8))
    finally:
        dev.free()
        Pp.close(); Pc.close()
    for b in range(B):
        rp, rs, _ = oracle.fb_klt(oracle.Pyramid(prevs[b], 9, 3), oracle.Pyramid(curs[b], 9, 3), 9, nbpyrlvl, 30.0, 0.5, kps[b], pri[b])
        assert np.array_equal(gs[b].astype(bool), rs) and np.all(gs[b] <= 1), (b, "status")
        assert np.array_equal(gp[b].view(np.uint32), rp.view(np.uint32)), (b, "positions")
        assert rs.sum() >= N // 2, (b, int(rs.sum()))                          # the case tracks: not a comparison of failures
