"""Local-map matching on the GPU (k_map_match<false>, csrc/mapmatch.hip, ov2_match_to_map[_batch]) against the numpy specification
(tests/match_ref.py, flat()): every output array bit-exact for the undistorted and the radial-tangential calibrations -- status bytes, indices, the
float distances and projections --, the crafted quirks, the batch form against single calls, an EuRoC-sized keyframe whose rows
exceed 64 observers, byte-identical repeats, the fisheye model to 1 float ulp of the projection on margin-filtered scenes, and the
C++ adapter (ov2slam_amd/host/mapper.hpp) against the Python form."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from ov2slam_amd import _lib as L
from ov2slam_amd import mapper
from tests import match_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("lm_status", "lm_kp", "lm_dist", "lm_projpx", "kp_lm", "kp_dist")
CALIBS = {"nodist": dict(D=None), "radtan4": dict(D=R.RADTAN4), "radtan5": dict(D=R.RADTAN5)}


def _check(got, ref, ulp=0):
    ok, field = R.same(got, ref, projpx_ulp=ulp)
    if not ok:
        bad = np.nonzero(np.asarray(got[field]).reshape(len(got[field]), -1) != np.asarray(ref[field]).reshape(len(ref[field]), -1))[0] \
            if field != "n_matches" else []
        raise AssertionError("%s differs at rows %s: got %s, want %s" % (field, bad[:8], np.asarray(got[field])[bad[:8]] if len(bad) else
                                                                         got[field], np.asarray(ref[field])[bad[:8]] if len(bad) else ref[field]))


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("nb3d", [20, 100])
@pytest.mark.parametrize("calib", list(CALIBS))
def test_bit_exact_against_specification(gpu_ctx, calib, nb3d, seed):
    P = R.make_params(**CALIBS[calib])
    M = R.make_scene(P, np.random.default_rng(7 + 10 * seed + nb3d), nb3dkps=nb3d, n_kp=150, n_lm=400)
    kf, _ = R.flatten(M)
    ref = R.flat(P, kf)
    got = mapper.match_to_map(gpu_ctx, P, kf)
    _check(got, ref)
    assert ref["n_matches"] > 5 and (ref["lm_status"] == R.RATIO_REJECTED).any()


@pytest.mark.parametrize("case", R.crafted_cases(), ids=lambda c: c[0])
def test_crafted_quirks_bit_exact(gpu_ctx, case):
    name, M, status, lm_kp = case
    kf, _ = R.flatten(M)
    got = mapper.match_to_map(gpu_ctx, M["params"], kf)
    assert [int(s) for s in got["lm_status"]] == status
    assert [int(k) for k in got["lm_kp"]] == lm_kp
    _check(got, R.flat(M["params"], kf))


def _empty_kf(P):
    nbw, nbh = R.grid_width(P)
    z = lambda *s: np.zeros(s, np.int32)
    return dict(Tcw=np.array([0, 0, 0, 0, 0, 0, 1.0]), nb3dkps=0, kp_px=np.zeros((0, 2), np.float32), kp_mp=z(0),
                cell_start=z(nbw * nbh + 1), cell_kp=z(0), obs_start=z(1), obs_kfid=z(0), obs_kf=z(0),
                obs_px=np.zeros((0, 2), np.float32), desc_start=z(1), desc=np.zeros((0, 32), np.uint8), kf_Tcw=np.zeros((0, 7)),
                lm_mp=z(0), lm_wpt=np.zeros((0, 3)))


def test_batch_of_11_equals_single_calls(gpu_ctx):
    P = R.make_params(D=R.RADTAN4)
    rng = np.random.default_rng(11)
    kfs = []
    for b in range(11):
        if b == 4:
            kfs.append(_empty_kf(P))
            continue
        M = R.make_scene(P, rng, nb3dkps=20 if b % 3 == 0 else 100, n_kp=int(rng.integers(1, 200)), n_lm=int(rng.integers(1, 500)),
                         many_obs=2 if b == 7 else 0)
        kfs.append(R.flatten(M)[0])
    no_kp = dict(kfs[1]); no_kp.update(kp_px=np.zeros((0, 2), np.float32), kp_mp=np.zeros(0, np.int32),
                                        cell_start=np.zeros_like(kfs[1]["cell_start"]), cell_kp=np.zeros(0, np.int32))
    kfs[9] = no_kp                                                      # local map points but no keypoint
    got = mapper.match_to_map_batch(gpu_ctx, P, kfs)
    assert len(got) == 11
    for b, kf in enumerate(kfs):
        single = mapper.match_to_map(gpu_ctx, P, kf)
        for f in FIELDS:
            assert np.asarray(got[b][f]).tobytes() == np.asarray(single[f]).tobytes(), (b, f)
        assert got[b]["n_matches"] == single["n_matches"]
        _check(got[b], R.flat(P, kf))
    assert len(got[4]["lm_status"]) == 0 and got[4]["n_matches"] == 0
    assert got[9]["n_matches"] == 0 and (got[9]["lm_kp"] == -1).all()
    assert mapper.match_to_map_batch(gpu_ctx, P, []) == []


def test_euroc_sized_keyframe_and_identical_repeats(gpu_ctx):
    """3080 local map points x 308 keypoints, rows of up to 80 observers (the chunked sum), twice with identical bytes"""
    P = R.make_params(D=R.RADTAN4)
    M = R.make_scene(P, np.random.default_rng(3080), n_kp=308, n_lm=3200, many_obs=40, dup=0.7)
    kf, _ = R.flatten(M)
    assert len(kf["lm_mp"]) >= 3080 and int(np.diff(kf["obs_start"]).max()) > 64
    ref = R.flat(P, kf)
    big = np.diff(kf["obs_start"])[kf["kp_mp"][ref["lm_kp"][ref["lm_kp"] >= 0]]]
    assert (big > 64).any(), "no accepted candidate with more than 64 observers: the chunked sum is not exercised"
    a = mapper.match_to_map(gpu_ctx, P, kf)
    b = mapper.match_to_map(gpu_ctx, P, kf)
    _check(a, ref)
    for f in FIELDS:
        assert np.asarray(a[f]).tobytes() == np.asarray(b[f]).tobytes(), f


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fisheye_projection_within_one_ulp_everything_else_exact(gpu_ctx, seed):
    """atan on the device may differ from the host's in the last bit: 1 float ulp on lm_projpx, everything else exact, on scenes
    whose gate quantities all lie at least 1e-3 px from their thresholds in the reference form (the generator resamples)"""
    P = R.make_params(D=R.FISHEYE4, model="fisheye")
    M, kf, meta, ref = R.filtered_scene(P, seed, min_margin=1e-3, n_kp=150, n_lm=400, nb3dkps=20 if seed == 1 else 100)
    got = mapper.match_to_map(gpu_ctx, P, kf)
    _check(got, ref, ulp=1)
    assert ref["n_matches"] > 5


def test_invalid_arguments_leave_the_outputs(gpu_ctx):
    P = R.make_params()
    kf = R.flatten(R.make_scene(P, np.random.default_rng(2), n_kp=40, n_lm=80))[0]
    s, keep, n_lm, n_kp = mapper._match_keyframe(kf)
    r, out = mapper._match_result(n_lm, n_kp)
    p = mapper._as_match_params(P)
    lib = gpu_ctx.lib
    assert lib.ov2_match_to_map(gpu_ctx.h, C.byref(p), C.byref(s), C.byref(r)) == L.OV2_OK
    before = {f: out[f].copy() for f in FIELDS}
    for f in FIELDS:
        out[f].view(np.uint8)[...] = 0xEE
    bad = dict(kf); bad["lm_mp"] = kf["lm_mp"].copy(); bad["lm_mp"][0] = len(kf["obs_start"]) - 1
    s2, keep2, _, _ = mapper._match_keyframe(bad)
    assert lib.ov2_match_to_map(gpu_ctx.h, C.byref(p), C.byref(s2), C.byref(r)) == L.OV2_EINVAL
    assert lib.ov2_match_to_map(None, C.byref(p), C.byref(s), C.byref(r)) == L.OV2_EINVAL
    assert lib.ov2_match_to_map_batch(gpu_ctx.h, C.byref(p), 70000, C.byref(s), C.byref(r)) == L.OV2_EUNSUPPORTED
    assert all((out[f].view(np.uint8) == 0xEE).all() for f in FIELDS), "a rejected call wrote its outputs"
    assert lib.ov2_match_to_map(gpu_ctx.h, C.byref(p), C.byref(s), C.byref(r)) == L.OV2_OK
    for f in FIELDS:
        assert out[f].tobytes() == before[f].tobytes(), f


def _wr(f, a):
    a = np.ascontiguousarray(a)
    f.write(struct.pack("<q", a.nbytes)); f.write(a.tobytes())


def _rd(f, dt):
    nb = struct.unpack("<q", f.read(8))[0]
    return np.frombuffer(f.read(nb), dt)


def test_cpp_adapter(gpu_ctx, tmp_path):
    """tests/cpp/match_run.cpp: ov2::Mapper::matchToMap and matchToMapBatch return the Python form's map_previd_newid"""
    exe = tmp_path / "match_run"
    libdir = os.path.join(ROOT, "ov2slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "match_run.cpp"),
                           "-o", str(exe), "-L", libdir, "-lov2slam_hip", "-Wl,-rpath," + libdir])
    P = R.make_params(D=R.RADTAN5)
    M = R.make_scene(P, np.random.default_rng(44), n_kp=200, n_lm=500)
    kf, meta = R.flatten(M)
    case, res = tmp_path / "case.bin", tmp_path / "res.bin"
    with open(case, "wb") as f:
        _wr(f, np.array([L.OV2_CAM_PINHOLE, P["ncellsize"], kf["nb3dkps"]], np.int32))
        _wr(f, np.array([P["fmax_proj_pxdist"], P["fmax_desc_dist"]], np.float32))
        _wr(f, np.array(list(P["K"]) + [P["img_w"], P["img_h"]], np.float64))
        _wr(f, np.array(P["D"], np.float64))
        _wr(f, kf["Tcw"]); _wr(f, np.array(meta["kp_lmid"], np.int32)); _wr(f, kf["kp_px"]); _wr(f, kf["kp_mp"])
        _wr(f, kf["cell_start"]); _wr(f, kf["cell_kp"]); _wr(f, kf["obs_start"]); _wr(f, kf["obs_kfid"]); _wr(f, kf["obs_kf"])
        _wr(f, kf["obs_px"]); _wr(f, kf["desc_start"]); _wr(f, kf["desc"]); _wr(f, kf["kf_Tcw"])
        _wr(f, np.array(meta["lm_lmid"], np.int32)); _wr(f, kf["lm_mp"]); _wr(f, kf["lm_wpt"])
    r = subprocess.run([str(exe), str(case), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    py = mapper.match_to_map(gpu_ctx, P, kf)
    want = {meta["kp_lmid"][k]: meta["lm_lmid"][l] for k, l in enumerate(py["kp_lm"]) if l >= 0}
    assert len(want) > 5 and want == R.replay(M)[0]
    with open(res, "rb") as f:
        for form in ("single", "batch"):
            kp_lm, st, kv = _rd(f, np.int32), _rd(f, np.uint8), _rd(f, np.int32).reshape(-1, 2)
            assert np.array_equal(kp_lm, py["kp_lm"]) and np.array_equal(st, py["lm_status"]), form
            assert {int(a): int(b) for a, b in kv} == want, form
