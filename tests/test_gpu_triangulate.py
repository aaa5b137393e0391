"""Keyframe triangulation on the GPU (csrc/triangulate.hip, ov2_triangulate_keyframe[_batch]): every branch bit-exact against the
numpy restatement (tests/tri_ref.py) -- wpt and invdepth as uint64, status bytes, NaN as a mask --, the batch form against single
calls, argument checks, a stereo-matching -> computeKeypoints -> triangulation chain on a plane of known depth, and the C++
adapter (ov2slam_amd/host/mapper.hpp) against the Python form."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import ov2slam_amd
from ov2slam_amd import _lib as L
from ov2slam_amd import mapper, stereo, synth
from tests import tri_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_f64(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def _check(got, ref):
    st, w, inv = ref
    assert np.array_equal(got["status"], st), np.nonzero(got["status"] != st)
    assert _same_f64(got["wpt"], w)
    assert _same_f64(got["invdepth"], inv)
    c = got["counts"]
    assert c["n_stereo"] == int(((st & R.ST_STEREO_TRIED) > 0).sum()) and c["n_stereo_good"] == int(((st & R.ST_STEREO_OK) > 0).sum())
    assert c["n_candidates"] == int(((st & R.ST_TEMPORAL_TRIED) > 0).sum())
    assert c["n_temporal_good"] == int(((st & R.ST_TEMPORAL_OK) > 0).sum())


# (name, camera, stereo, rect, n, n_src)
SCENES = [
    ("euroc_unrect_rotated_extrinsic", R.EUROC, True, False, 308, 4),
    ("kitti_rect", R.KITTI, True, True, 300, 3),
    ("mono_temporal", R.EUROC, False, False, 250, 5),
    ("many_source_keyframes", R.EUROC, True, False, 500, 40),
    ("n_65", R.KITTI, True, True, 65, 2),
    ("n_1", R.EUROC, True, False, 1, 1),
]


def _scene(cam, st, rect, n, n_src, seed):
    P = R.make_params(cam, stereo=st, rect=rect, seed=seed, rot=0.03)
    M = R.make_map(P, np.random.default_rng(seed), n=n, n_src=n_src, noise=0.4, behind=0.05, no_motion_kf=seed % 2 == 1,
                   kps_3d=0.05, lone=0.1, missing_src_kp=0.05, motion=0.3)
    return P, R.inputs_from_map(M)[0]


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("scene", SCENES, ids=lambda s: s[0])
def test_bit_exact_against_restatement(gpu_ctx, scene, seed):
    _, cam, st, rect, n, n_src = scene
    P, kf = _scene(cam, st, rect, n, n_src, 10 * seed + n_src)
    got = mapper.triangulate_keyframe(gpu_ctx, P, kf)
    ref = R.keyframe(P, kf)
    _check(got, ref)
    if n >= 64:
        assert (ref[0] & R.ST_STEREO_OK if st else ref[0] & R.ST_TEMPORAL_OK).any()


@pytest.mark.parametrize("case", R.crafted_cases(), ids=lambda c: c[0])
def test_crafted_branches_bit_exact(gpu_ctx, case):
    name, P, kf, expected = case
    got = mapper.triangulate_keyframe(gpu_ctx, P, kf)
    assert int(got["status"][0]) == expected
    _check(got, R.keyframe(P, kf))


def test_empty_keyframe(gpu_ctx):
    P = R.make_params()
    kf = dict(Twc=np.array([0, 0, 0, 0, 0, 0, 1.0]), unpx=np.zeros((0, 2), np.float32), bv=np.zeros((0, 3)))
    got = mapper.triangulate_keyframe(gpu_ctx, P, kf)
    assert len(got["status"]) == 0 and got["counts"]["n_candidates"] == 0


def _kfs(n_items, seed, empty_every=5):
    rng = np.random.default_rng(seed)
    P = R.make_params(R.EUROC, stereo=True, rect=False, seed=seed)
    base = []
    for k in range(6):
        M = R.make_map(P, rng, n=int(rng.integers(1, 320)), n_src=int(rng.integers(1, 6)), noise=0.4, behind=0.05, no_motion_kf=k == 2)
        base.append(R.inputs_from_map(M)[0])
    empty = dict(Twc=np.array([0, 0, 0, 0, 0, 0, 1.0]), unpx=np.zeros((0, 2), np.float32), bv=np.zeros((0, 3)))
    return P, [empty if b % empty_every == 3 else base[b % len(base)] for b in range(n_items)]


@pytest.mark.parametrize("n_items", [1, 11, 1100])
def test_batch_equals_single_calls(gpu_ctx, n_items):
    P, kfs = _kfs(n_items, n_items)
    got = mapper.triangulate_keyframe_batch(gpu_ctx, P, kfs)
    assert len(got) == n_items
    singles = {}
    for b, kf in enumerate(kfs):
        key = id(kf)
        if key not in singles:
            singles[key] = mapper.triangulate_keyframe(gpu_ctx, P, kf)
        s = singles[key]
        assert np.array_equal(got[b]["status"], s["status"]) and _same_f64(got[b]["wpt"], s["wpt"]), b
        assert _same_f64(got[b]["invdepth"], s["invdepth"]) and got[b]["counts"] == s["counts"], b
    for kf in kfs[:12]:
        _check(singles[id(kf)], R.keyframe(P, kf))


def test_batch_of_zero_items(gpu_ctx):
    assert mapper.triangulate_keyframe_batch(gpu_ctx, R.make_params(), []) == []


def test_invalid_arguments(gpu_ctx):
    P, kf = _scene(R.EUROC, True, False, 20, 2, 3)
    lib = gpu_ctx.lib
    s, keep, n = mapper._keyframe(kf)
    r, out = mapper._result(n)
    p = mapper._as_params(P)

    def call(s_=None, r_=None, p_=None, ctx=gpu_ctx.h):
        return lib.ov2_triangulate_keyframe(ctx, C.byref(p_ or p), C.byref(s_ or s), C.byref(r_ or r))

    assert call() == L.OV2_OK
    assert call(ctx=None) == L.OV2_EINVAL
    assert lib.ov2_triangulate_keyframe(gpu_ctx.h, None, C.byref(s), C.byref(r)) == L.OV2_EINVAL
    assert lib.ov2_triangulate_keyframe_batch(gpu_ctx.h, C.byref(p), -1, C.byref(s), C.byref(r)) == L.OV2_EINVAL
    before = out["status"].copy()
    out["status"][:] = 0xEE
    bad = mapper._keyframe(kf)[0]; bad.n = -1
    assert call(s_=bad) == L.OV2_EINVAL
    rr = mapper._result(n)[0]; rr.wpt = None
    assert call(r_=rr) == L.OV2_EINVAL
    k2 = dict(kf); k2["src"] = kf["src"].copy(); k2["src"][0] = len(kf["src_Twc"])      # one past the table
    assert call(s_=mapper._keyframe(k2)[0]) == L.OV2_EINVAL
    k3 = dict(kf); k3["src"] = kf["src"].copy(); k3["src"][0] = -2
    assert call(s_=mapper._keyframe(k3)[0]) == L.OV2_EINVAL
    k4 = dict(kf); k4["is_stereo"] = np.ones(n, np.uint8); k4["runpx"] = None
    assert call(s_=mapper._keyframe(k4)[0]) == L.OV2_EINVAL
    k5 = dict(kf); k5["is_stereo"] = np.ones(n, np.uint8); k5["rbv"] = None
    assert call(s_=mapper._keyframe(k5)[0]) == L.OV2_EINVAL
    Pm = dict(P); Pm["stereo"] = False
    k6 = dict(kf); k6["is_stereo"] = np.ones(n, np.uint8)
    assert call(s_=mapper._keyframe(k6)[0], p_=mapper._as_params(Pm)) == L.OV2_EINVAL
    assert (out["status"] == 0xEE).all(), "a rejected call wrote its outputs"
    assert call() == L.OV2_OK and np.array_equal(out["status"], before)


def test_stereo_match_to_triangulation_chain(gpu_ctx):
    """ov2_stereo_match on a rectified pair of a fronto-parallel plane (disparity 20 px), the right points through
    ov2_compute_keypoints, then the rectified stereo pass: depths within 1 % of fx b / 20"""
    w, h, disp = 752, 480, 20
    tex = synth.base_texture(max(w, h) + 400, 23)
    l, r = tex[50:50 + h, 100:100 + w].copy(), tex[50:50 + h, 100 + disp:100 + disp + w].copy()
    K = (458.654, 458.654, 367.215, 248.375)
    cal = ov2slam_amd.CameraCalibration(gpu_ctx, "pinhole", *K, D=None)
    pl = ov2slam_amd.Pyramid(gpu_ctx, w, h, 9, 3).build(l)
    pr = ov2slam_amd.Pyramid(gpu_ctx, w, h, 9, 3).build(r)
    trk = ov2slam_amd.FeatureTracker(gpu_ctx, 30, 0.01)
    kps = synth.grid_keypoints(w, h, 35, np.random.default_rng(8))[:300]
    kps = kps[kps[:, 0] > 40]
    unpx, bv = cal.computeKeypoints(kps)
    ok, right = stereo.stereo_matching_fused(trk, pl, pr, kps, unpx, cal, rect=True)
    assert ok.mean() > 0.85
    runpx, rbv = cal.computeKeypoints(right)
    b = 0.11
    Tlr = np.array([b, 0, 0, 0, 0, 0, 1.0])
    P = mapper.tri_params(K, cal.iK, K, Tlr, R._inv7(Tlr), stereo=True, rect=True, fmax_reproj_err=3.0)
    n = len(kps)
    kf = dict(Twc=np.array([0, 0, 0, 0, 0, 0, 1.0]), unpx=unpx, bv=bv, is_stereo=ok.astype(np.uint8), runpx=runpx, rbv=rbv)
    got = mapper.triangulate_keyframe(gpu_ctx, P, kf)
    good = (got["status"] & mapper.STEREO_OK) > 0
    assert good.sum() >= 0.85 * n
    z = got["wpt"][good, 2]
    assert np.abs(z / (K[0] * b / disp) - 1).max() < 0.01, np.abs(z / (K[0] * b / disp) - 1).max()
    assert np.allclose(got["invdepth"][good], 1 / z, rtol=1e-12)
    Pd = dict(stereo=True, rect=True, fmax_reproj_err=3.0, K=K, iK=cal.iK.reshape(9), Kr=K, Tlr=Tlr, Tcic0=R._inv7(Tlr))
    kf.update(src=np.full(n, -1, np.int32), src_unpx=np.zeros((n, 2), np.float32), src_bv=np.zeros((n, 3)),
              src_Twc=np.zeros((0, 7)), src_Tcw=np.zeros((0, 7)))
    _check(got, R.keyframe(Pd, kf))


def _wr(f, a):
    a = np.ascontiguousarray(a)
    f.write(struct.pack("<q", a.nbytes)); f.write(a.tobytes())


def _rd(f, dt):
    nb = struct.unpack("<q", f.read(8))[0]
    return np.frombuffer(f.read(nb), dt)


def test_cpp_adapter(gpu_ctx, tmp_path):
    """tests/cpp/tri_run.cpp: ov2::Mapper::triangulate and triangulateBatch return the Python form's results, and its actions
    equal the restatement's replay order"""
    exe = tmp_path / "tri_run"
    libdir = os.path.join(ROOT, "ov2slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "tri_run.cpp"),
                           "-o", str(exe), "-L", libdir, "-lov2slam_hip", "-Wl,-rpath," + libdir])
    P = R.make_params(R.EUROC, stereo=True, rect=False, seed=4)
    M = R.make_map(P, np.random.default_rng(44), n=300, n_src=5, noise=0.4, behind=0.05)
    kf, lmids, table = R.inputs_from_map(M)
    case, res = tmp_path / "case.bin", tmp_path / "res.bin"
    with open(case, "wb") as f:
        _wr(f, np.array([int(P["stereo"]), int(P["rect"]), M["frame"]["kfid"]], np.int32))
        _wr(f, np.array([P["fmax_reproj_err"]], np.float32))
        _wr(f, np.concatenate([np.asarray(P[k], np.float64).reshape(-1) for k in ("K", "iK", "Kr", "Tlr", "Tcic0")]))
        _wr(f, kf["Twc"]); _wr(f, np.array(lmids, np.int32)); _wr(f, kf["unpx"]); _wr(f, kf["bv"]); _wr(f, kf["is_stereo"])
        _wr(f, kf["runpx"]); _wr(f, kf["rbv"]); _wr(f, kf["src"]); _wr(f, kf["src_unpx"]); _wr(f, kf["src_bv"])
        _wr(f, np.array(table, np.int32)); _wr(f, kf["src_Twc"]); _wr(f, kf["src_Tcw"])
    r = subprocess.run([str(exe), str(case), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    py = mapper.triangulate_keyframe(gpu_ctx, P, kf)
    with open(res, "rb") as f:
        for form in ("single", "batch"):
            st, w, inv = _rd(f, np.uint8), _rd(f, np.float64).reshape(-1, 3), _rd(f, np.float64)
            assert np.array_equal(st, py["status"]) and _same_f64(w, py["wpt"]) and _same_f64(inv, py["invdepth"]), form
            acts = _rd(f, np.float64).reshape(-1, 7)        # op, lmid, kfid, wpt[3], invdepth
            ref = R.replay(P, __import__("copy").deepcopy(M))
            assert len(acts) == len(ref), form
            names = {0: "rm_stereo", 1: "update", 2: "rm_obs"}
            for a, b in zip(acts, ref):
                assert names[int(a[0])] == b[0] and int(a[1]) == b[1], (form, a, b)
                if b[0] == "update":
                    assert R._bits(a[3:6]) == b[2] and R._bits([a[6]]) == b[3]
                    src = kf["src"][lmids.index(b[1])]
                    st_i = py["status"][lmids.index(b[1])]
                    want = M["frame"]["kfid"] if st_i & R.ST_STEREO_OK else table[src]
                    assert int(a[2]) == want
                elif b[0] == "rm_obs":
                    assert int(a[2]) == b[2]
