"""GPU parity tests (through the C ABI) of the HIP grid detectors against the oracle.
Bar: keypoint sets bit-exact (integer pixel coordinates) and sub-pixel coordinates bit-exact
(float32 bits), adaptive thresholds identical."""
import numpy as np
import pytest

import ov2slam_amd
from ov2slam_amd import synth
from ov2slam_amd import _lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["cell", "strip"], autouse=True)
def mineig_kernel(request, gpu_ctx):
    """Every test of this file runs with both response kernels of detectSingleScale -- one wavefront per cell (k_mineig_cells) and the
    batch form (k_mineig_strip: the free cells of an image as one strip of columns, several cells per work-group) -- pinned through
    OV2_OPT_DETECT_STRIP; left alone the library picks by launch size and single images would only see the first."""
    with gpu_ctx.options(detect_strip=1 if request.param == "strip" else 0):
        yield request.param


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _images():
    out = []
    a, _, _ = synth.frame_pair(752, 480, seed=8)
    out.append(("euroc", a))
    b, _, _ = synth.frame_pair(1241, 376, seed=13)
    out.append(("kitti", b))
    rng = np.random.default_rng(3)
    out.append(("noise", rng.integers(0, 256, (480, 752), dtype=np.uint8)))
    return out


IMAGES = _images()


@pytest.mark.parametrize("name", [n for n, _ in IMAGES])
@pytest.mark.parametrize("cell", [50, 35, 58, 64])
@pytest.mark.parametrize("mode", [L.OV2_MASK_AS_EXECUTED, L.OV2_MASK_INTENDED])
def test_grid_fast_bit_exact(gpu_ctx, oracle, name, cell, mode):
    img = dict(IMAGES)[name]
    rng = np.random.default_rng(17)
    h, w = img.shape
    cur = synth.grid_keypoints(w, h, cell, rng)[::3]                  # a third of the cells already occupied
    for subpix in (False, True):
        fx = ov2slam_amd.FeatureExtractor(gpu_ctx, nfast_th=10, mask_mode=mode)
        g = fx.detectGridFAST(img, cell, cur, subpix=subpix)
        r, rth = oracle.detect_grid_fast(img, cell, cur, 10, mode, subpix=subpix)
        assert g.shape == r.shape, (g.shape, r.shape)
        assert np.array_equal(_bits(g), _bits(r))
        assert fx.nfast_th_ == rth
    assert len(r) > 10


@pytest.mark.parametrize("tie", [L.OV2_FAST_TIE_SCAN_ORDER, L.OV2_FAST_TIE_LIBSTDCXX])
def test_grid_fast_ties_among_equal_responses(gpu_ctx, oracle, tie):
    """detectGridFAST's std::sort (src/feature_extractor.cpp:518): with more than 16 corners left in a cell the winner among EQUAL best
    responses is the standard library's choice.  OV2_OPT_FAST_TIE selects libstdc++'s introsort restated on the device (what the reference
    built with g++ does -- tests/test_reference_factors.py runs the reference's own source against the oracle's copy of it) or the first
    in scan order; both against the oracle in the same mode, bit for bit, at thresholds that leave many corners per cell."""
    prev = gpu_ctx.get_option(L.OV2_OPT_FAST_TIE)
    gpu_ctx.set_option(L.OV2_OPT_FAST_TIE, tie)
    n_diff = 0
    try:
        for name, img in IMAGES:
            h, w = img.shape
            rng = np.random.default_rng(23)
            for cell in (35, 50, 64):
                cur = synth.grid_keypoints(w, h, cell, rng)[::4]
                for th0 in (5, 9, 20):
                    for mode in (L.OV2_MASK_AS_EXECUTED, L.OV2_MASK_INTENDED):
                        fx = ov2slam_amd.FeatureExtractor(gpu_ctx, nfast_th=th0, mask_mode=mode)
                        g = fx.detectGridFAST(img, cell, cur, subpix=False)
                        with oracle.fast_tie_mode(tie):
                            r, rth = oracle.detect_grid_fast(img, cell, cur, th0, mode, subpix=False)
                        assert g.shape == r.shape and np.array_equal(_bits(g), _bits(r)), (name, cell, th0, mode, int((g != r).any(1).sum()) if g.shape == r.shape else -1)
                        assert fx.nfast_th_ == rth
                        with oracle.fast_tie_mode(1 - tie):
                            o, _ = oracle.detect_grid_fast(img, cell, cur, th0, mode, subpix=False)
                        n_diff += int((o != r).any(1).sum()) if o.shape == r.shape else 1
    finally:
        gpu_ctx.set_option(L.OV2_OPT_FAST_TIE, prev)
    assert n_diff > 20 and oracle.fast_tie_sort_fallbacks() == 0        # the two modes do differ on these inputs: the test bites


@pytest.mark.parametrize("name", [n for n, _ in IMAGES])
@pytest.mark.parametrize("cell", [35, 45, 53, 58, 63, 64])
def test_singlescale_bit_exact(gpu_ctx, oracle, name, cell):
    img = dict(IMAGES)[name]
    h, w = img.shape
    roi = (5, 5, w - 10, h - 10)                                      # camera_calibration.cpp:72-73
    rng = np.random.default_rng(19)
    for cur in (np.zeros((0, 2), np.float32), synth.grid_keypoints(w, h, cell, rng)[::2]):
        for subpix in (False, True):
            fx = ov2slam_amd.FeatureExtractor(gpu_ctx, dmaxquality=0.001)
            g = fx.detectSingleScale(img, cell, cur, roi, subpix=subpix)
            r, rq = oracle.detect_singlescale(img, cell, cur, roi, 0.001, subpix=subpix)
            assert g.shape == r.shape, (g.shape, r.shape)
            assert np.array_equal(_bits(g), _bits(r))
            assert fx.dmaxquality_ == rq
    assert len(r) > 10


def test_threshold_adaptation_sequence(gpu_ctx, oracle):
    """Run the detectors repeatedly like successive keyframes: the adaptive state must follow
    the oracle step by step (nfast_th_: :546-552, dmaxquality_: :418-423)."""
    img = dict(IMAGES)["euroc"]
    fx = ov2slam_amd.FeatureExtractor(gpu_ctx, nfast_th=40, dmaxquality=0.02, mask_mode=L.OV2_MASK_INTENDED)
    th, q = 40, 0.02
    none = np.zeros((0, 2), np.float32)
    for _ in range(5):
        g = fx.detectGridFAST(img, 50, none, subpix=False)
        r, th = oracle.detect_grid_fast(img, 50, none, th, L.OV2_MASK_INTENDED, subpix=False)
        assert np.array_equal(g, r) and fx.nfast_th_ == th
        g2 = fx.detectSingleScale(img, 35, none, (5, 5, 742, 470), subpix=False)
        r2, q = oracle.detect_singlescale(img, 35, none, (5, 5, 742, 470), q, subpix=False)
        assert np.array_equal(g2, r2) and fx.dmaxquality_ == q


def test_detect_edge_cases(gpu_ctx, oracle):
    fx = ov2slam_amd.FeatureExtractor(gpu_ctx)
    # empty image -> empty result (:291-294 / :446-449)
    assert fx.detectGridFAST(np.zeros((0, 0), np.uint8), 35, np.zeros((0, 2))).shape == (0, 2)
    assert fx.detectSingleScale(np.zeros((0, 0), np.uint8), 35, np.zeros((0, 2)), (0, 0, 0, 0)).shape == (0, 2)
    # flat image: nothing detected, thresholds decay like the oracle's
    flat = np.full((480, 752), 128, np.uint8)
    g = fx.detectGridFAST(flat, 50, np.zeros((0, 2)))
    r, th = oracle.detect_grid_fast(flat, 50, np.zeros((0, 2), np.float32), 10)
    assert len(g) == 0 and len(r) == 0 and fx.nfast_th_ == th
    g = fx.detectSingleScale(flat, 35, np.zeros((0, 2)), (5, 5, 742, 470))
    r, q = oracle.detect_singlescale(flat, 35, np.zeros((0, 2), np.float32), (5, 5, 742, 470), 0.001)
    assert len(g) == 0 and len(r) == 0 and fx.dmaxquality_ == q
    # every cell occupied
    img = dict(IMAGES)["euroc"]
    cur = synth.grid_keypoints(752, 480, 35, np.random.default_rng(0), jitter=0.1)
    assert len(fx.detectSingleScale(img, 35, cur, (5, 5, 742, 470))) == 0
    # image smaller than one cell row/col of slack: cells that fail the in-image test are skipped
    small = np.ascontiguousarray(img[:71, :106])
    fx2 = ov2slam_amd.FeatureExtractor(gpu_ctx)
    g = fx2.detectSingleScale(small, 35, np.zeros((0, 2)), (5, 5, 96, 61), subpix=False)
    r, _ = oracle.detect_singlescale(small, 35, np.zeros((0, 2), np.float32), (5, 5, 96, 61), 0.001, subpix=False)
    assert np.array_equal(g, r)


def test_corner_subpix_bit_exact_including_border(gpu_ctx, oracle):
    img = dict(IMAGES)["euroc"]
    rng = np.random.default_rng(23)
    pts = np.stack([rng.uniform(0, 751, 600), rng.uniform(0, 479, 600)], 1).astype(np.float32)
    pts[:40, 0] = rng.uniform(0, 6, 40); pts[40:80, 1] = rng.uniform(474, 479.9, 40)      # generic (border) sampler path
    pts[80:120] = np.rint(pts[80:120])
    fx = ov2slam_amd.FeatureExtractor(gpu_ctx)
    g = fx.cornerSubPix(img, pts)
    r = oracle.corner_subpix(img, pts)
    assert np.array_equal(_bits(g), _bits(r))
    assert np.abs(g - pts).max() <= 3.0 + 1e-6


@pytest.mark.parametrize("order", [L.OV2_SOBEL_DY_OPENCV_ROWFILTER, L.OV2_SOBEL_DY_EXACT_SUM])
def test_singlescale_sobel_dy_orders_bit_exact(oracle, order):
    """Both evaluation orders of cv::Sobel(dx=0, dy=1, scale) (ov2_ctx_set_option / oracle.set_sobel_dy_order): the HIP
    detector follows the oracle bit for bit in either, on the noise image (the one with the most arg-max near-ties)."""
    ctx = ov2slam_amd.Context(0)
    ctx.set_option(L.OV2_OPT_SOBEL_DY_ORDER, order)
    prev = oracle.set_sobel_dy_order(order)
    try:
        for name, img in IMAGES:
            h, w = img.shape
            roi = (5, 5, w - 10, h - 10)
            fx = ov2slam_amd.FeatureExtractor(ctx, dmaxquality=0.001)
            g = fx.detectSingleScale(img, 35, np.zeros((0, 2), np.float32), roi)
            r, q = oracle.detect_singlescale(img, 35, np.zeros((0, 2), np.float32), roi, 0.001)
            assert len(g) == len(r) and np.array_equal(_bits(g), _bits(r)), name
            assert fx.dmaxquality_ == q
    finally:
        oracle.set_sobel_dy_order(prev)
        ctx.close()
    with pytest.raises(ov2slam_amd.Ov2Error):
        c2 = ov2slam_amd.Context(0)
        try:
            c2.set_option(L.OV2_OPT_SOBEL_DY_ORDER, 7)
        finally:
            c2.close()


@pytest.mark.parametrize("wh", [(752, 480), (1241, 376)])
def test_device_resident_detectors_read_pyramid_level0(gpu_ctx, oracle, wh):
    """ov2_detect_*_d on level 0 of the tracker's current pyramid (the CLAHE'd keyframe image, map_manager.cpp:312-320):
    same points as the host-image entry points and as the oracle on the equalised image; thresholds adapt identically."""
    w, h = wh
    img, _, _ = synth.frame_pair(w, h, seed=17)
    trk = ov2slam_amd.VisualFrontEndTracker(gpu_ctx, w, h, use_clahe=True, fclahe_val=3.0, nbmaxkps=64)
    trk.trackFrame(img, np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), None)
    eq = oracle.clahe(img, 3.0, w // 50, h // 50)
    roi = (5, 5, w - 10, h - 10)
    rng = np.random.default_rng(4)
    cur = synth.grid_keypoints(w, h, 35, rng)[::3]
    for curkps in (np.zeros((0, 2), np.float32), cur):
        fa, fb = ov2slam_amd.FeatureExtractor(gpu_ctx, dmaxquality=0.001), ov2slam_amd.FeatureExtractor(gpu_ctx, dmaxquality=0.001)
        g = fa.detectSingleScalePyr(trk.cur_pyr, 35, curkps, roi)
        hst = fb.detectSingleScale(eq, 35, curkps, roi)
        r, q = oracle.detect_singlescale(eq, 35, curkps, roi, 0.001)
        assert len(g) == len(r) and np.array_equal(_bits(g), _bits(r)) and np.array_equal(_bits(g), _bits(hst))
        assert fa.dmaxquality_ == q == fb.dmaxquality_
        fa = ov2slam_amd.FeatureExtractor(gpu_ctx, nfast_th=10)
        g = fa.detectGridFASTPyr(trk.cur_pyr, 50, curkps)
        r, th = oracle.detect_grid_fast(eq, 50, curkps, 10)
        assert len(g) == len(r) and np.array_equal(_bits(g), _bits(r)) and fa.nfast_th_ == th
    trk.close()


_BATCH_DETECT_SCRIPT = r"""
import ctypes as C, os, sys, numpy as np
import torch
torch.cuda.init()
sys.path.insert(0, sys.argv[1])
import ov2slam_amd
from ov2slam_amd import synth
ctx = ov2slam_amd.Context(0)
B, W, H, CELL, NCUR = 11, 376, 240, 35, 48            # 11 items: one pass (DET_CHUNK = 1024 items, in two sets of 512) -- the pass loop runs below with 1100 items
rng = np.random.default_rng(5)
imgs, curs, ncur = [], np.zeros((B, NCUR, 2), np.float32), np.zeros(B, np.int32)
for b in range(B):
    img, _, _ = synth.frame_pair(W, H, seed=90 + b)
    if b == 3: img = np.full_like(img, 128)                       # a flat image: nothing to detect
    imgs.append(img)
    k = synth.grid_keypoints(W, H, CELL, rng)
    n = [0, 5, 48, 17][b % 4]
    curs[b, :n] = k[:n]; ncur[b] = n
P = ov2slam_amd.Pyramid(ctx, W, H, 9, 0, batch=B).build(np.stack(imgs))
ctx.sync()
ncells = (W // CELL) * (H // CELL)
roi = (5, 5, W - 10, H - 10)
d_cur = torch.from_numpy(curs).cuda(); d_n = torch.from_numpy(ncur).cuda()
for subpix in (True, False):
    # ---- single scale ----
    cap = 2 * ncells + 3
    d_out = torch.full((B, cap, 2), -7.0, dtype=torch.float32, device="cuda")
    q = np.array([1e-3, 1e-2, 1e-4, 1e-3, 0.5, 1e-3, 1e-3, 1e-5, 1e-3, 1e-3, 1e-2], np.float64)
    q0 = q.copy()
    torch.cuda.synchronize()
    n = ov2slam_amd.FeatureExtractor.detectSingleScaleBatch(ctx, P, CELL, d_cur.data_ptr(), NCUR, d_n.data_ptr(), roi, q, d_out.data_ptr(), cap, subpix=subpix)
    out = d_out.cpu().numpy()
    for b in range(B):
        fx = ov2slam_amd.FeatureExtractor(ctx, dmaxquality=float(q0[b]))
        ref = fx.detectSingleScale(imgs[b], CELL, curs[b, :ncur[b]], roi, subpix=subpix)
        assert n[b] == len(ref), ("singlescale count", b, n[b], len(ref))
        assert np.array_equal(out[b, :n[b]].view(np.uint32), ref.view(np.uint32)), ("singlescale", b)
        assert np.all(out[b, 2 * ncells:] == -7.0), "slots beyond the list capacity must stay untouched"
        assert q[b] == fx.dmaxquality_, ("quality adaptation", b, q[b], fx.dmaxquality_)
    assert n[3] == 0 and n.sum() > 100
    # ---- FAST, both mask modes ----
    for mode in (ov2slam_amd._lib.OV2_MASK_AS_EXECUTED, ov2slam_amd._lib.OV2_MASK_INTENDED):
        cap = ncells
        d_out = torch.full((B, cap, 2), -7.0, dtype=torch.float32, device="cuda")
        th = np.array([10, 20, 5, 10, 40, 7, 10, 10, 3, 10, 60], np.int32)
        th0 = th.copy()
        torch.cuda.synchronize()
        n = ov2slam_amd.FeatureExtractor.detectGridFASTBatch(ctx, P, CELL, d_cur.data_ptr(), NCUR, d_n.data_ptr(), th, d_out.data_ptr(), cap, mask_mode=mode, subpix=subpix)
        out = d_out.cpu().numpy()
        for b in range(B):
            fx = ov2slam_amd.FeatureExtractor(ctx, nfast_th=int(th0[b]), mask_mode=mode)
            ref = fx.detectGridFAST(imgs[b], CELL, curs[b, :ncur[b]], subpix=subpix)
            assert n[b] == len(ref), ("fast count", b, n[b], len(ref))
            assert np.array_equal(out[b, :n[b]].view(np.uint32), ref.view(np.uint32)), ("fast", b)
            assert th[b] == fx.nfast_th_, ("threshold adaptation", b)
# no current keypoints at all (NULL lists)
cap = 2 * ncells
d_out = torch.zeros((B, cap, 2), dtype=torch.float32, device="cuda"); q = np.full(B, 1e-3)
torch.cuda.synchronize()
n = ov2slam_amd.FeatureExtractor.detectSingleScaleBatch(ctx, P, CELL, 0, 0, 0, roi, q, d_out.data_ptr(), cap)
out = d_out.cpu().numpy()
for b in (0, 7):
    ref = ov2slam_amd.FeatureExtractor(ctx, dmaxquality=1e-3).detectSingleScale(imgs[b], CELL, np.zeros((0, 2), np.float32), roi)
    assert n[b] == len(ref) and np.array_equal(out[b, :n[b]].view(np.uint32), ref.view(np.uint32))
# more items than one pass holds: beyond 512 items the passes (512 each, two scratch sets) alternate between the context's stream and an
# auxiliary one -- 1100 items = three passes (main, auxiliary, main); items cycle through the 11 images AND their keypoint lists / thresholds
B2 = 1100
idx = np.arange(B2) % B
P2 = ov2slam_amd.Pyramid(ctx, W, H, 9, 0, batch=B2).build(np.stack([imgs[i] for i in idx]))
d_cur2 = torch.from_numpy(np.ascontiguousarray(curs[idx])).cuda(); d_n2 = torch.from_numpy(np.ascontiguousarray(ncur[idx])).cuda()
cap = 2 * ncells
d_out = torch.zeros((B2, cap, 2), dtype=torch.float32, device="cuda")
qb = np.array([1e-3, 1e-2, 1e-4, 1e-3, 0.5, 1e-3, 1e-3, 1e-5, 1e-3, 1e-3, 1e-2], np.float64)
q1 = qb.copy(); q2 = qb[idx].copy()
d_ref = torch.zeros((B, cap, 2), dtype=torch.float32, device="cuda")
torch.cuda.synchronize()
n1 = ov2slam_amd.FeatureExtractor.detectSingleScaleBatch(ctx, P, CELL, d_cur.data_ptr(), NCUR, d_n.data_ptr(), roi, q1, d_ref.data_ptr(), cap)
n2 = ov2slam_amd.FeatureExtractor.detectSingleScaleBatch(ctx, P2, CELL, d_cur2.data_ptr(), NCUR, d_n2.data_ptr(), roi, q2, d_out.data_ptr(), cap)
ref, out2 = d_ref.cpu().numpy(), d_out.cpu().numpy()
for i in range(B2):
    assert n2[i] == n1[i % B] and q2[i] == q1[i % B], ("multi-pass batch: count / adapted quality", i)
    assert np.array_equal(out2[i, :n2[i]].view(np.uint32), ref[i % B, :n2[i]].view(np.uint32)), ("multi-pass batch", i)
d_out = torch.zeros((B2, ncells, 2), dtype=torch.float32, device="cuda"); d_ref = torch.zeros((B, ncells, 2), dtype=torch.float32, device="cuda")
thb = np.array([10, 20, 5, 10, 40, 7, 10, 10, 3, 10, 60], np.int32)
t1 = thb.copy(); t2 = thb[idx].copy()
torch.cuda.synchronize()
n1 = ov2slam_amd.FeatureExtractor.detectGridFASTBatch(ctx, P, CELL, d_cur.data_ptr(), NCUR, d_n.data_ptr(), t1, d_ref.data_ptr(), ncells)
n2 = ov2slam_amd.FeatureExtractor.detectGridFASTBatch(ctx, P2, CELL, d_cur2.data_ptr(), NCUR, d_n2.data_ptr(), t2, d_out.data_ptr(), ncells)
ref, out2 = d_ref.cpu().numpy(), d_out.cpu().numpy()
for i in range(B2):
    assert n2[i] == n1[i % B] and t2[i] == t1[i % B], ("multi-pass FAST batch: count / adapted threshold", i)
    assert np.array_equal(out2[i, :n2[i]].view(np.uint32), ref[i % B, :n2[i]].view(np.uint32)), ("multi-pass FAST batch", i)
# the context's stream is usable right after (the auxiliary stream was joined): a single-image call gives the usual answer
ref0 = ov2slam_amd.FeatureExtractor(ctx, dmaxquality=1e-3).detectSingleScale(imgs[0], CELL, np.zeros((0, 2), np.float32), roi)
assert len(ref0) == n[0]
print("BATCH_DETECT_OK")
"""


def test_batched_device_resident_detectors():
    """ov2_detect_singlescale_batch_d / ov2_detect_grid_fast_batch_d: every batch item of a pyramid in one call, device-resident
    keypoint lists in and out, per-item adaptive state -- identical, item by item, to the single-image forms (which the tests above
    pin to the oracle).  Own process: torch owns the device buffers and has to initialise HIP first."""
    import os, subprocess, sys
    pytest.importorskip("torch")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _BATCH_DETECT_SCRIPT, root], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "BATCH_DETECT_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]



@pytest.mark.parametrize("tie", [L.OV2_FAST_TIE_SCAN_ORDER, L.OV2_FAST_TIE_LIBSTDCXX])
def test_grid_fast_720p_sort_areas_share_the_lds(gpu_ctx, oracle, tie):
    """on 1280x720 at cell 35 the exclusion mask and cell tables take ~133 KB of the 160 KB LDS; the sort areas of the
    libstdc++ tie order are carved out of what is left (fewer than one per wavefront, taken under a lock) instead of a static 37 KB
    that made the launch fail.  A low threshold on noise leaves many equal responses per cell, so the sort path runs."""
    rng = np.random.default_rng(41)
    base, _, _ = synth.frame_pair(1280, 720, seed=21)
    noise = rng.integers(0, 256, (720, 1280), dtype=np.uint8)
    prev = gpu_ctx.get_option(L.OV2_OPT_FAST_TIE)
    gpu_ctx.set_option(L.OV2_OPT_FAST_TIE, tie)
    try:
        for img, th0 in ((base, 10), (noise, 5), (noise, 20)):
            cur = synth.grid_keypoints(1280, 720, 35, rng)[::4]
            for mode in (L.OV2_MASK_AS_EXECUTED, L.OV2_MASK_INTENDED):
                fx = ov2slam_amd.FeatureExtractor(gpu_ctx, nfast_th=th0, mask_mode=mode)
                g = fx.detectGridFAST(img, 35, cur, subpix=False)
                with oracle.fast_tie_mode(tie):
                    r, rth = oracle.detect_grid_fast(img, 35, cur, th0, mode, subpix=False)
                assert g.shape == r.shape and np.array_equal(_bits(g), _bits(r)) and fx.nfast_th_ == rth
                assert len(r) > 100
    finally:
        gpu_ctx.set_option(L.OV2_OPT_FAST_TIE, prev)
    # an image whose mask alone exceeds the LDS is refused with OV2_EUNSUPPORTED, not a launch failure
    big = rng.integers(0, 256, (1200, 1920), dtype=np.uint8)
    with pytest.raises(ov2slam_amd.Ov2Error) as e:
        ov2slam_amd.FeatureExtractor(gpu_ctx, nfast_th=10).detectGridFAST(big, 35, np.zeros((0, 2), np.float32), subpix=False)
    assert e.value.code == L.OV2_EUNSUPPORTED
