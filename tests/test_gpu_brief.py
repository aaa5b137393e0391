"""describeBRIEF on the GPU (csrc/brief.hip, k_brief32): every call form bit-exact against the numpy restatement (tests/brief_ref.py)
-- 32 bytes and the valid flag per point."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import ov2slam_amd
from ov2slam_amd import _lib as L
from ov2slam_amd import synth
from tests import brief_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _builtin():
    txt = open(os.path.join(ROOT, "ov2slam_amd", "csrc", "brief_pattern.hpp")).read()
    body = txt[txt.index("= {") + 3:txt.index("};")]
    return np.array([int(v) for v in re.findall(r"-?\d+", body)], np.int8).reshape(256, 4)


def _random_pattern(seed):
    rng = np.random.default_rng(seed)
    p = rng.integers(-24, 25, (256, 4)).astype(np.int8)
    p[0] = (24, 24, -24, -24); p[1] = (-24, 24, 24, -24); p[2] = (0, 24, 0, 24); p[3] = (24, -24, 24, 23)
    return p


def _strided(img, pad=13):
    """the same pixels in a buffer whose rows are longer than the image (stride != width)"""
    h, w = img.shape
    buf = np.full((h, w + pad), 77, np.uint8)
    buf[:, :w] = img
    return buf[:, :w]


def _points(w, h, rng, n_rand=300):
    pts = [synth.grid_keypoints(w, h, 35, rng), np.stack([rng.uniform(-10, w + 10, n_rand), rng.uniform(-10, h + 10, n_rand)], 1)]
    band = []
    for v in np.arange(27.0, 29.01, 0.25):
        band += [(v, h / 2), (w / 2, v), (v, v)]
    for v in np.arange(w - 30.0, w - 26.99, 0.25):
        band.append((v, h / 2 + 1))
    for v in np.arange(h - 30.0, h - 26.99, 0.25):
        band.append((w / 2 + 1, v))
    half = [(27.5, 27.5), (28.5, 28.5), (w - 28.5, h / 2), (w / 2, h - 28.5), (w - 28.5, h - 28.5), (w - 29.5, h - 29.5),
            (100.5, 60.5), (101.5, 61.5)]
    bad = [(-5.0, 40.0), (40.0, -3.0), (np.nan, 40.0), (40.0, np.nan), (np.inf, 40.0), (-np.inf, -np.inf), (1e30, 40.0)]
    out = np.concatenate([p for p in pts] + [np.array(band, np.float64).reshape(-1, 2), np.array(half), np.array(bad)])
    out = out.astype(np.float32)
    dup = out[rng.integers(0, len(out), 20)]
    return np.concatenate([out, dup]).astype(np.float32)


def _images():
    e = synth.frame_pair(752, 480, seed=5)[1]
    k = synth.frame_pair(1241, 376, seed=6)[0]
    rng = np.random.default_rng(3)
    return [("euroc", e), ("kitti", k), ("noise", rng.integers(0, 256, (300, 257), dtype=np.uint8)),
            ("const", np.full((200, 180), 131, np.uint8)), ("tiny57", rng.integers(0, 256, (57, 57), dtype=np.uint8)),
            ("odd", rng.integers(0, 256, (121, 99), dtype=np.uint8))]


@pytest.mark.parametrize("pattern", ["builtin", "random"])
def test_host_form_matches_restatement(gpu_ctx, pattern):
    fx = ov2slam_amd.FeatureExtractor(gpu_ctx)
    pat = _builtin() if pattern == "builtin" else _random_pattern(9)
    gpu_ctx.set_brief_pattern(None if pattern == "builtin" else pat)
    try:
        assert np.array_equal(gpu_ctx.brief_pattern(), pat)
        rng = np.random.default_rng(17)
        for name, img in _images():
            h, w = img.shape
            pts = _points(w, h, rng)
            view = _strided(img)
            assert view.strides[0] != w
            d, v = fx.describeBRIEF(view, pts)
            rd, rv = R.describe(img, pts, pat)
            assert np.array_equal(v, rv), name
            assert np.array_equal(d, rd), name
            if name == "const":
                assert not d.any()
            if w > 56 and h > 56:
                assert v.sum() > 0, name
            if name in ("kitti", "odd"):      # rule 5: odd width, x == W-28.5 survives and its +24 boxes stop at the image edge
                assert v[np.flatnonzero(pts[:, 0] == np.float32(w - 28.5))].any()
    finally:
        gpu_ctx.set_brief_pattern(None)


def test_pattern_set_get(gpu_ctx):
    lib = gpu_ctx.lib
    p = _random_pattern(1)
    gpu_ctx.set_brief_pattern(p)
    bad = p.copy(); bad[100, 2] = 25
    assert lib.ov2_brief_set_pattern(gpu_ctx.h, bad.ctypes.data) == L.OV2_EINVAL
    bad[100, 2] = -25
    assert lib.ov2_brief_set_pattern(gpu_ctx.h, bad.ctypes.data) == L.OV2_EINVAL
    assert np.array_equal(gpu_ctx.brief_pattern(), p)                      # the previous table is kept
    img = synth.frame_pair(320, 240, seed=2)[0]
    pts = synth.grid_keypoints(320, 240, 35, np.random.default_rng(0))
    d, v = ov2slam_amd.FeatureExtractor(gpu_ctx).describeBRIEF(img, pts)
    rd, rv = R.describe(img, pts, p)
    assert np.array_equal(d, rd) and np.array_equal(v, rv)
    gpu_ctx.set_brief_pattern(None)
    assert np.array_equal(gpu_ctx.brief_pattern(), _builtin())
    with pytest.raises(ValueError):
        gpu_ctx.set_brief_pattern(np.full((256, 4), 25))


def test_empty_and_small_images(gpu_ctx):
    fx = ov2slam_amd.FeatureExtractor(gpu_ctx)
    img = np.random.default_rng(1).integers(0, 256, (100, 120), dtype=np.uint8)
    d, v = fx.describeBRIEF(img, np.zeros((0, 2), np.float32))
    assert d.shape == (0, 32) and v.shape == (0,)
    assert gpu_ctx.lib.ov2_describe_brief(gpu_ctx.h, None, 0, 0, 0, None, 0, None, None) == L.OV2_OK     # n == 0: nothing is read
    for w, h in ((56, 100), (100, 56), (56, 56), (57, 200)):
        im = np.random.default_rng(w + h).integers(0, 256, (h, w), dtype=np.uint8)
        pts = np.array([[28, 28], [w / 2, h / 2], [28.4, 28.4]], np.float32)
        d, v = fx.describeBRIEF(_strided(im), pts)
        rd, rv = R.describe(im, pts, _builtin())
        assert np.array_equal(d, rd) and np.array_equal(v, rv)
        assert v.any() == (w > 56 and h > 56)


def test_tracker_form_reads_the_raw_frame(gpu_ctx):
    w, h = 752, 480
    prev, cur, _ = synth.frame_pair(w, h, seed=8)
    vt = ov2slam_amd.VisualFrontEndTracker(gpu_ctx, w, h, use_clahe=True, fclahe_val=3.0)
    try:
        rng = np.random.default_rng(4)
        pts = _points(w, h, rng)
        fx = ov2slam_amd.FeatureExtractor(gpu_ctx)
        for img in (prev, cur):
            vt.trackFrame(img, np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), None)
            d, v = vt.describeBRIEF(pts)
            hd, hv = fx.describeBRIEF(img, pts)
            assert np.array_equal(d, hd) and np.array_equal(v, hv)
            rd, rv = R.describe(img, pts, _builtin())
            assert np.array_equal(d, rd) and np.array_equal(v, rv)
            clahe, _ = vt.cur_pyr.download(0)
            assert not np.array_equal(clahe, img)
            cd, _ = fx.describeBRIEF(clahe, pts)
            assert not np.array_equal(cd[v], d[v])                        # it describes imraw, not the CLAHE'd level 0
        vt.preprocessImage(prev)                                           # asynchronous preprocess: same stream, same answer
        d, v = vt.describeBRIEF(pts)
        assert np.array_equal(d, R.describe(prev, pts, _builtin())[0])
        assert vt.describeBRIEF(np.zeros((0, 2), np.float32))[0].shape == (0, 32)
    finally:
        vt.close()


def _batch_case(B, w, h, cap, seed):
    rng = np.random.default_rng(seed)
    tex = synth.base_texture(seed=seed)
    imgs = np.stack([synth.frame_pair(w, h, tex=tex, shift=(7.3 * b, -4.1 * b), theta=0.01 * b)[1] for b in range(B)])
    imgs[B // 2] = rng.integers(0, 256, (h, w), dtype=np.uint8)
    n = rng.integers(0, cap + 1, B).astype(np.int32)
    n[0], n[1], n[2] = 0, cap, cap
    pts = np.zeros((B, cap, 2), np.float32)
    for b in range(B):
        p = _points(w, h, rng, n_rand=cap)
        pts[b] = p[rng.permutation(len(p))[:cap]]
    return imgs, pts, n


_BATCH_SCRIPT = r"""
import sys
import numpy as np
import torch
torch.cuda.init()                      # torch's HIP runtime must be initialised before libov2slam_hip.so in one process
sys.path.insert(0, sys.argv[1])
import ov2slam_amd
from tests.test_gpu_brief import _batch_case
B, w, h, cap = 64, 200, 150, 96
imgs, pts, n = _batch_case(B, w, h, cap, 3)
pitch, stride = 256, 256 * h + 512
buf = np.zeros((B, stride), np.uint8)
for b in range(B):
    buf[b, :pitch * h].reshape(h, pitch)[:, :w] = imgs[b]
ctx = ov2slam_amd.Context(0)
d_img = torch.from_numpy(buf).cuda()
d_pts = torch.from_numpy(pts).cuda(); d_n = torch.from_numpy(n).cuda()
d_desc = torch.full((B, cap, 32), 0xAB, dtype=torch.uint8, device="cuda")
d_valid = torch.full((B, cap), 7, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
ov2slam_amd.FeatureExtractor.describeBRIEFBatch(ctx, d_img.data_ptr(), w, h, pitch, stride, B, d_pts.data_ptr(), cap,
                                                d_n.data_ptr(), d_desc.data_ptr(), d_valid.data_ptr())
fx = ov2slam_amd.FeatureExtractor(ctx)
host_d = np.zeros((B, cap, 32), np.uint8); host_v = np.zeros((B, cap), bool)
for b in range(B):
    host_d[b, :n[b]], host_v[b, :n[b]] = fx.describeBRIEF(imgs[b], pts[b, :n[b]])
np.savez(sys.argv[2], desc=d_desc.cpu().numpy(), valid=d_valid.cpu().numpy(), host_d=host_d, host_v=host_v)
ctx.close()
print("batch script ok")
"""


def test_batch_d_matches_host_form(tmp_path):
    """ov2_describe_brief_batch_d on torch-owned HBM (its own process: torch's runtime initialises first there)"""
    import sys
    pytest.importorskip("torch")
    out = tmp_path / "batch.npz"
    r = subprocess.run([sys.executable, "-c", _BATCH_SCRIPT, ROOT, str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and "batch script ok" in r.stdout, r.stderr[-3000:]
    z = np.load(out)
    desc, valid, host_d, host_v = z["desc"], z["valid"], z["host_d"], z["host_v"]
    B, w, h, cap = 64, 200, 150, 96
    imgs, pts, n = _batch_case(B, w, h, cap, 3)
    assert 0 in n and cap in n
    for b in range(B):
        k = int(n[b])
        assert np.array_equal(desc[b, :k], host_d[b, :k]) and np.array_equal(valid[b, :k].astype(bool), host_v[b, :k]), b
        assert np.all(desc[b, k:] == 0xAB) and np.all(valid[b, k:] == 7), b            # slots past n[b] are not written
        rd, rv = R.describe(imgs[b], pts[b, :k], _builtin())
        assert np.array_equal(desc[b, :k], rd) and np.array_equal(valid[b, :k].astype(bool), rv), b


def test_btracker_form(gpu_ctx):
    B, w, h, cap = 64, 200, 150, 96
    imgs, pts, n = _batch_case(B, w, h, cap, 4)
    lt = ov2slam_amd.LockstepTracker(gpu_ctx, B, w, h, use_clahe=True, nbmaxkps=64)
    try:
        with pytest.raises(ov2slam_amd.Ov2Error):
            lt.describeBRIEF(B, pts, n)                                     # no step yet
        for b in range(B):
            lt.image_buffers[0][b][:, :w] = imgs[b]
        z = np.zeros((B, 64, 2), np.float32)
        lt.trackFrame(lt.image_buffers[0], z, z, None, np.zeros(B, np.int32))
        desc, valid = lt.describeBRIEF(B, pts, n)
        fx = ov2slam_amd.FeatureExtractor(gpu_ctx)
        for b in range(B):
            k = int(n[b])
            hd, hv = fx.describeBRIEF(imgs[b], pts[b, :k])
            assert np.array_equal(desc[b, :k], hd) and np.array_equal(valid[b, :k], hv), b
            assert not desc[b, k:].any() and not valid[b, k:].any()
        d2, v2 = lt.describeBRIEF(10, pts, n[:10])                         # a prefix of the step's items
        assert np.array_equal(d2, desc[:10]) and np.array_equal(v2, valid[:10])
        lt.upload(1, B)                                                     # another staging set: the current frames stay
        d3, _ = lt.describeBRIEF(B, pts, n)
        assert np.array_equal(d3, desc)
        lt.upload(0, B)                                                     # the set holding the current frames is re-uploaded
        with pytest.raises(ov2slam_amd.Ov2Error) as e:
            lt.describeBRIEF(B, pts, n)
        assert e.value.code == L.OV2_EINVAL
    finally:
        lt.close()


def _wr(f, a):
    b = np.ascontiguousarray(a).tobytes()
    f.write(struct.pack("<q", len(b))); f.write(b)


def _rd(f, dt):
    (k,) = struct.unpack("<q", f.read(8))
    return np.frombuffer(f.read(k), dt).copy()


def test_cpp_adapter(gpu_ctx, tmp_path):
    exe = tmp_path / "brief_run"
    libdir = os.path.join(ROOT, "ov2slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "brief_run.cpp"),
                           "-o", str(exe), "-L", libdir, "-lov2slam_hip", "-Wl,-rpath," + libdir])
    w, h = 752, 480
    img = synth.frame_pair(w, h, seed=21)[0]
    pts = _points(w, h, np.random.default_rng(21))
    case, res = tmp_path / "case.bin", tmp_path / "res.bin"
    with open(case, "wb") as f:
        _wr(f, np.array([w, h], np.int32)); _wr(f, img); _wr(f, pts)
    r = subprocess.run([str(exe), str(case), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rd, rv = R.describe(img, pts, _builtin())
    with open(res, "rb") as f:
        for form in ("host", "tracker", "abi"):
            d = _rd(f, np.uint8).reshape(-1, 32); v = _rd(f, np.uint8).astype(bool)
            assert np.array_equal(d, rd) and np.array_equal(v, rv), form
        assert int(_rd(f, np.int32)[0]) == 0
