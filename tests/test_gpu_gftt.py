"""detectGFTT on the GPU (csrc/gftt.hip): every call form bit-exact against the numpy restatement (tests/gftt_ref.py) -- point
bits and counts -- and the forms against each other."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import ov2slam_amd
from ov2slam_amd import _lib as L
from ov2slam_amd import synth
from tests import gftt_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w)).astype(np.uint8)


def _plateau(w, h):
    img = np.full((h, w), 40, np.uint8)
    img[6:h - 6:9, 6:w - 6:9] = 220            # equal isolated dots: equal response peaks (ties)
    return img


def _roi(w, h, b=5):
    m = np.zeros((h, w), np.uint8)
    m[b:h - b, b:w - b] = 255
    return m


def _strided(a, pad=11, fill=3):
    h, w = a.shape
    buf = np.full((h, w + pad), fill, np.uint8)
    buf[:, :w] = a
    return buf[:, :w]


def _cur(w, h, n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n)], 1).astype(np.float32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# (name, w, h, image, ncur, roi, nbmax, nmaxpts, nmaxdist, dmaxquality, subpix, dy order)
CASES = [
    ("euroc", 752, 480, "frame", 0, True, -1, 308, 35, 0.001, 1, 0),
    ("euroc_cur", 752, 480, "frame", 120, True, -1, 400, 17, 0.01, 1, 0),
    ("kitti", 1241, 376, "frame", 60, False, -1, 300, 35, 0.001, 1, 1),
    ("noise", 640, 480, "noise", 0, False, 150, 400, 17, 0.01, 0, 0),
    ("small_nbmax", 376, 240, "frame", 30, True, 12, 300, 20, 0.01, 1, 0),
    ("pass2", 320, 200, "frame", 10, False, -1, 300, 20, 0.01, 1, 0),
    ("pass2_dy1", 320, 200, "frame", 10, True, -1, 300, 20, 0.01, 0, 1),
    ("constant", 200, 150, "constant", 0, False, -1, 100, 10, 0.01, 1, 0),
    ("plateau", 240, 160, "plateau", 0, False, -1, 200, 9, 0.01, 0, 0),
    ("plateau_sub", 240, 160, "plateau", 5, True, 50, 200, 14, 0.01, 1, 1),
    ("full", 320, 200, "frame", 400, False, -1, 300, 35, 0.01, 1, 0),
]


def _case(c):
    name, w, h, kind, ncur, roi, nbmax, nmaxpts, nmaxdist, q, sub, dy = c
    seed = sum(map(ord, name)) % 1000
    if kind == "frame":
        img = synth.frame_pair(w, h, seed=seed)[0]
    elif kind == "noise":
        img = _noise(w, h, seed)
    elif kind == "constant":
        img = np.full((h, w), 128, np.uint8)
    else:
        img = _plateau(w, h)
    cur = _cur(w, h, ncur, seed + 1)
    return img, cur, _roi(w, h) if roi else None


@pytest.mark.parametrize("c", CASES, ids=[c[0] for c in CASES])
def test_host_form_matches_restatement(gpu_ctx, c):
    name, w, h, kind, ncur, roi_on, nbmax, nmaxpts, nmaxdist, q, sub, dy = c
    img, cur, roi = _case(c)
    fx = ov2slam_amd.FeatureExtractor(gpu_ctx, dmaxquality=q, nmaxpts=nmaxpts, nmaxdist=nmaxdist)
    gpu_ctx.set_option(L.OV2_OPT_SOBEL_DY_ORDER, dy)
    try:
        got = fx.detectGFTT(_strided(img), cur, None if roi is None else _strided(roi, fill=0), nbmax=nbmax, subpix=bool(sub))
    finally:
        gpu_ctx.set_option(L.OV2_OPT_SOBEL_DY_ORDER, 0)
    info = {}
    ref = R.detect_gftt(img, cur, roi, nbmax, R.params(nmaxpts, nmaxdist, q), subpix=bool(sub), dy_order=dy, info=info)
    assert _same(got, ref), (name, len(got), len(ref))
    if kind in ("constant",) or ncur >= nmaxpts:
        assert len(got) == 0
    else:
        assert len(got) > 0
    if name == "euroc":
        print("euroc candidates (pass 1):", info["ncand"])


@pytest.mark.parametrize("name,taken", [("pass2", True), ("pass2_dy1", True), ("euroc", True), ("small_nbmax", False),
                                        ("noise", False), ("plateau_sub", False)])
def test_cases_cover_both_pass2_branches(name, taken):
    """the host-form cases above include both outcomes of the pass-2 rule (decided by the restatement on the same inputs)"""
    c = [c for c in CASES if c[0] == name][0]
    _, w, h, kind, ncur, roi_on, nbmax, nmaxpts, nmaxdist, q, sub, dy = c
    img, cur, roi = _case(c)
    info = {}
    R.detect_gftt(img, cur, roi, nbmax, R.params(nmaxpts, nmaxdist, q), subpix=bool(sub), dy_order=dy, info=info)
    assert info["pass2"] is taken


def test_pyramid_form_equals_host_form(gpu_ctx):
    w, h = 752, 480
    img = synth.frame_pair(w, h, seed=31)[0]
    cur = _cur(w, h, 80, 32)
    fx = ov2slam_amd.FeatureExtractor(gpu_ctx, dmaxquality=0.005, nmaxpts=300, nmaxdist=25)
    P = ov2slam_amd.Pyramid(gpu_ctx, w, h, 9, 3).build(img)
    for roi in (None, _roi(w, h)):
        for sub in (True, False):
            a = fx.detectGFTTPyr(P, cur, roi, subpix=sub)
            b = fx.detectGFTT(img, cur, roi, subpix=sub)
            assert _same(a, b) and len(a) > 0


def _raw(fx, img, cur, nbmax, cap, roi=None, w=None, h=None):
    h0, w0 = img.shape
    w = w0 if w is None else w
    h = h0 if h is None else h
    out = np.zeros((max(cap, 1), 2), np.float32)
    n = C.c_int(-5)
    p = fx.gftt_params()
    rc = fx.lib.ov2_detect_gftt(fx.ctx.h, img.ctypes.data_as(C.c_void_p), w, h, w0, None, 0, C.byref(p),
                                cur.ctypes.data_as(C.c_void_p), len(cur), nbmax, 1, out.ctypes.data_as(C.c_void_p), cap, C.byref(n))
    return rc, n.value, out


def test_invalid_arguments(gpu_ctx):
    img = synth.frame_pair(200, 150, seed=4)[0]
    cur = np.zeros((0, 2), np.float32)
    fx = ov2slam_amd.FeatureExtractor(gpu_ctx, nmaxpts=100, nmaxdist=10)
    assert _raw(fx, img, cur, 0, 100)[0] == L.OV2_EINVAL
    assert _raw(fx, img, cur, -2, 100)[0] == L.OV2_EINVAL
    assert _raw(fx, img, cur, -1, 99)[0] == L.OV2_EINVAL            # nb2detect 100
    assert _raw(fx, img, cur, 30, 29)[0] == L.OV2_EINVAL
    rc, n, _ = _raw(fx, img, cur, 30, 30)
    assert rc == 0 and 0 < n <= 30
    rc, n, _ = _raw(fx, img, cur, -1, 100, w=0)                       # empty image
    assert rc == 0 and n == 0
    with pytest.raises(ov2slam_amd.Ov2Error):
        fx.detectGFTT(img, cur, nbmax=0)
    assert len(fx.detectGFTT(np.zeros((0, 0), np.uint8), cur)) == 0


_BATCH_SCRIPT = r"""
import os, sys, numpy as np
import torch
torch.cuda.init()
sys.path.insert(0, sys.argv[1])
import ov2slam_amd
from ov2slam_amd import synth
ctx = ov2slam_amd.Context(0)
B, W, H, NCUR = 150, 376, 240, 64           # ~2 MB of scratch per item: a 256 MB chunk holds fewer than 150 items
fx = ov2slam_amd.FeatureExtractor(ctx, dmaxquality=0.01, nmaxpts=200, nmaxdist=20)
rng = np.random.default_rng(8)
base = [synth.frame_pair(W, H, seed=200 + k)[0] for k in range(6)]
imgs = np.stack([np.roll(base[b % 6], (b * 7) % 50, axis=b % 2) for b in range(B)])
imgs[5] = 128
curs = np.zeros((B, NCUR, 2), np.float32); ncur = np.zeros(B, np.int32)
nb = np.array([[-1, 40, 12, -1, 150][b % 5] for b in range(B)], np.int32)
for b in range(B):
    k = np.stack([rng.uniform(0, W - 1, NCUR), rng.uniform(0, H - 1, NCUR)], 1)
    n = [0, 20, 64, 7, 0][b % 5]
    if b == 9: n = NCUR
    curs[b, :n] = k[:n]; ncur[b] = n
P = ov2slam_amd.Pyramid(ctx, W, H, 9, 0, batch=B).build(imgs)
ctx.sync()
roi = np.zeros((H, W), np.uint8); roi[5:H - 5, 5:W - 5] = 255
cap = 200 + 3
for use_roi in (True, False):
    d_roi = torch.from_numpy(roi).cuda()
    d_cur = torch.from_numpy(curs).cuda(); d_n = torch.from_numpy(ncur).cuda()
    d_out = torch.full((B, cap, 2), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    n = ov2slam_amd.FeatureExtractor.detectGFTTBatch(ctx, P, d_roi.data_ptr() if use_roi else 0, W, fx.gftt_params(), d_cur.data_ptr(), NCUR,
                                                     d_n.data_ptr(), nb, d_out.data_ptr(), cap)
    out = d_out.cpu().numpy()
    for b in list(range(0, 12)) + list(range(B - 12, B)) + [70, 71, 133, 134, 135]:
        ref = fx.detectGFTT(imgs[b], curs[b, :ncur[b]], roi if use_roi else None, nbmax=int(nb[b]))
        assert n[b] == len(ref), ("count", b, n[b], len(ref))
        assert np.array_equal(out[b, :n[b]].view(np.uint32), ref.view(np.uint32)), ("points", b)
        assert np.all(out[b, 200:] == -7.0), "slots beyond nb2detect are not written"
    assert n[5] == 0 and (n > 0).sum() > B // 2
    np.save(sys.argv[2], out[:12])
ctx.close()
print("batch script ok")
"""


def test_batch_d_matches_single_form(tmp_path):
    """ov2_detect_gftt_batch_d on torch-owned HBM across a chunk boundary (its own process: torch's runtime initialises first)"""
    pytest.importorskip("torch")
    out = tmp_path / "b.npy"
    r = subprocess.run([sys.executable, "-c", _BATCH_SCRIPT, ROOT, str(out)], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0 and "batch script ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_btracker_form(gpu_ctx):
    B, w, h, nmax = 12, 376, 240, 64
    lt = ov2slam_amd.LockstepTracker(gpu_ctx, B, w, h, use_clahe=True, nbmaxkps=nmax)
    try:
        for b in range(B):
            lt.image_buffers[0][b][:, :w] = synth.frame_pair(w, h, seed=300 + b)[0]
        z = np.zeros((B, nmax, 2), np.float32)
        lt.trackFrame(lt.image_buffers[0], z, z, None, np.zeros(B, np.int32))
        rng = np.random.default_rng(3)
        cur = np.zeros((B, nmax, 2), np.float32); ncur = np.array([0, 10, 64, 33] * 3, np.int32)
        for b in range(B):
            cur[b, :ncur[b]] = _cur(w, h, int(ncur[b]), 40 + b)
        fx = ov2slam_amd.FeatureExtractor(gpu_ctx, dmaxquality=0.01, nmaxpts=150, nmaxdist=20)
        nb = np.array([-1, 30, 10, -1] * 3, np.int32)
        roi = _roi(w, h)
        res = lt.detectGFTT(B, fx.gftt_params(), cur, ncur, nb, roi)
        for b in range(B):
            ref = fx.detectGFTTPyr(lt.cur_item(b), cur[b, :ncur[b]], roi, nbmax=int(nb[b]))
            assert _same(res[b], ref), b
        assert sum(len(r) for r in res) > 100
    finally:
        lt.close()


def _wr(f, a):
    b = np.ascontiguousarray(a).tobytes()
    f.write(struct.pack("<q", len(b))); f.write(b)


def _rd(f, dt):
    (k,) = struct.unpack("<q", f.read(8))
    return np.frombuffer(f.read(k), dt).copy()


@pytest.mark.parametrize("use_roi,nbmax", [(True, -1), (False, 40)])
def test_cpp_adapter_and_verbatim(gpu_ctx, tmp_path, use_roi, nbmax):
    """tests/cpp/gftt_run.cpp: ov2::FeatureExtractor::detectGFTT (host image and device pyramid) and the reference's own signature
    (ov2::verbatim::FeatureExtractor, -DOV2_WITH_OPENCV against tests/fake_opencv) return the Python form's points, bit for bit"""
    exe = tmp_path / "gftt_run"
    libdir = os.path.join(ROOT, "ov2slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-DOV2_WITH_OPENCV", "-I" + os.path.join(ROOT, "tests", "fake_opencv"),
                           os.path.join(ROOT, "tests", "cpp", "gftt_run.cpp"), "-o", str(exe), "-L", libdir, "-lov2slam_hip", "-Wl,-rpath," + libdir])
    w, h, stride, nmaxpts, nmaxdist, q = 752, 480, 760, 308, 35, 0.001
    img = synth.frame_pair(w, h, seed=21)[0]
    cur = _cur(w, h, 50, 22)
    roi = _roi(w, h) if use_roi else None
    buf = np.full((h, stride), 9, np.uint8); buf[:, :w] = img
    rbuf = np.zeros((h, stride), np.uint8)
    if use_roi:
        rbuf[:, :w] = roi
    case, res = tmp_path / "case.bin", tmp_path / "res.bin"
    with open(case, "wb") as f:
        _wr(f, np.array([w, h, stride, nmaxpts, nmaxdist, nbmax], np.int32)); _wr(f, np.array([q], np.float64))
        _wr(f, buf); _wr(f, rbuf if use_roi else np.zeros(0, np.uint8)); _wr(f, cur)
    r = subprocess.run([str(exe), str(case), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    fx = ov2slam_amd.FeatureExtractor(gpu_ctx, dmaxquality=q, nmaxpts=nmaxpts, nmaxdist=nmaxdist)
    py = fx.detectGFTT(img, cur, roi, nbmax=nbmax)
    assert len(py) > 0
    with open(res, "rb") as f:
        for form in ("host", "pyramid", "verbatim"):
            got = _rd(f, np.float32).reshape(-1, 2)
            assert _same(got, py), form
        nmindist, dminq_ok = _rd(f, np.int32)
        assert nmindist == nmaxdist // 2 and dminq_ok == 1
        assert _same(_rd(f, np.float32).reshape(-1, 2), py), "abi"
        assert list(_rd(f, np.int32)) == [0, 0]
