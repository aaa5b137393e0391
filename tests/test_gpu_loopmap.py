"""Loop local-map tracking on the GPU (k_map_match<true>, csrc/mapmatch.hip, ov2_loop_match_to_map[_batch]) against the numpy specification
(tests/loopmap_ref.py, flat()): every output array bit-exact for the undistorted and the radial-tangential calibrations -- status
bytes, indices, the float distances and projections --, the crafted shapes at which the kernel takes another path, the batch form
against single calls, an EuRoC-sized candidate with byte-identical repeats, the fisheye model to 1 float ulp of the projection on
margin-filtered scenes, rejected calls, the C++ adapter (ov2slam_amd/host/loop_closer.hpp) against the literal replay, and the
mapper's call (the kernel's other instantiation) on a scene where the two reference functions coincide."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from ov2slam_amd import _lib as L
from ov2slam_amd import loop_closer as LC
from ov2slam_amd import mapper
from tests import loopmap_ref as R
from tests import match_ref as MR

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


def _scene_261(P, rng):
    """n_kp = 120 asked for, exactly 261 local map points (not a multiple of the four wavefronts of a work-group), 8 keyframes"""
    M = R.make_scene(P, rng, n_kp=120, n_lm=340, n_kf=8, fov_points=8, matched=0.25)
    item, meta = R.flatten(M)
    assert len(item["lm_mp"]) >= 261
    return R.trim(item, meta, 261)


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("calib", list(CALIBS))
def test_bit_exact_against_specification(gpu_ctx, calib, seed):
    P = R.make_params(**CALIBS[calib])
    item, _ = _scene_261(P, np.random.default_rng(17 + seed))
    flagged = item["kp_matched"].mean()
    assert len(item["lm_mp"]) == 261 and 0.2 < flagged < 0.5
    ref = R.flat(P, item)
    got = LC.loop_match_to_map(gpu_ctx, P, item)
    _check(got, ref)
    assert ref["n_matches"] > 5 and (ref["lm_status"] == R.RATIO_REJECTED).any() and (ref["lm_status"] == R.OUT_OF_FOV).any()


@pytest.mark.parametrize("case", R.crafted_cases(), ids=lambda c: c[0])
def test_crafted_cases_bit_exact(gpu_ctx, case):
    name, M, status, lm_kp = case
    item, _ = R.flatten(M)
    got = LC.loop_match_to_map(gpu_ctx, M["params"], item)
    assert [int(s) for s in got["lm_status"]] == status
    assert [int(k) for k in got["lm_kp"]] == lm_kp
    _check(got, R.flat(M["params"], item))


@pytest.mark.parametrize("calib", list(CALIBS))
def test_agrees_with_the_mappers_call_where_the_functions_coincide(gpu_ctx, calib):
    """The device form of test_loopmap_reference's side-by-side test: no matched flags, nb3dkps >= 30, equal fmaxprojerr / fdistratio,
    every observation stale (the Mapper's re-projection gate then passes by its NaN rule), and without the points the Mapper's
    narrower viewing cone removes.  ov2_match_to_map and ov2_loop_match_to_map then return the same arrays, those of the
    specification: what the kernel's two instantiations share has stayed shared."""
    P = MR.make_params(fmax_proj_pxdist=10.0, fmax_desc_dist=R.FDISTRATIO, **CALIBS[calib])
    M = MR.make_scene(P, np.random.default_rng(5), n_kp=120, n_lm=261, nb3dkps=100)
    kf, _ = MR.flatten(M)
    kf["obs_kf"] = np.full_like(kf["obs_kf"], -1)
    kf["obs_px"] = np.zeros_like(kf["obs_px"])
    keep = MR.flat(P, kf)["lm_status"] != MR.OUT_OF_FOV
    assert 0 < (~keep).sum() < len(keep)
    kf["lm_mp"], kf["lm_wpt"] = kf["lm_mp"][keep], kf["lm_wpt"][keep]
    want = MR.flat(P, kf)
    item = {k: kf[k] for k in ("Tcw", "kp_px", "kp_mp", "cell_start", "cell_kp", "obs_start", "obs_kfid", "desc_start", "desc", "lm_mp", "lm_wpt")}
    item["kp_matched"] = np.zeros(len(kf["kp_mp"]), np.uint8)
    _check(R.flat(P, item), want)
    as_mapper = mapper.match_to_map(gpu_ctx, P, kf)
    as_loop = LC.loop_match_to_map(gpu_ctx, P, item)
    for f in FIELDS:
        assert np.asarray(as_mapper[f]).tobytes() == np.asarray(as_loop[f]).tobytes(), f
    assert as_mapper["n_matches"] == as_loop["n_matches"]
    _check(as_mapper, want)
    _check(as_loop, want)
    assert want["n_matches"] > 5 and (want["lm_status"] == R.RATIO_REJECTED).any() and not (as_loop["lm_status"] == R.OUT_OF_FOV).any()


def _empty_item(P):
    nbw, nbh = R.grid_width(P)
    z = lambda *s: np.zeros(s, np.int32)
    return dict(Tcw=np.array([0, 0, 0, 0, 0, 0, 1.0]), kp_px=np.zeros((0, 2), np.float32), kp_mp=z(0), kp_matched=np.zeros(0, np.uint8),
                cell_start=z(nbw * nbh + 1), cell_kp=z(0), obs_start=z(1), obs_kfid=z(0), desc_start=z(1),
                desc=np.zeros((0, 32), np.uint8), lm_mp=z(0), lm_wpt=np.zeros((0, 3)))


def test_batch_of_11_equals_single_calls(gpu_ctx):
    P = R.make_params(D=R.RADTAN4)
    rng = np.random.default_rng(11)
    items = []
    for b in range(11):
        if b == 4:
            items.append(_empty_item(P))
            continue
        M = R.make_scene(P, rng, n_kp=int(rng.integers(1, 150)), n_lm=int(rng.integers(1, 300)), many_obs=2 if b == 7 else 0)
        items.append(R.flatten(M)[0])
    no_kp = dict(items[1]); no_kp.update(kp_px=np.zeros((0, 2), np.float32), kp_mp=np.zeros(0, np.int32), kp_matched=np.zeros(0, np.uint8),
                                          cell_start=np.zeros_like(items[1]["cell_start"]), cell_kp=np.zeros(0, np.int32))
    items[9] = no_kp                                                    # local map points but no keypoint
    no_lm = dict(items[2]); no_lm.update(lm_mp=np.zeros(0, np.int32), lm_wpt=np.zeros((0, 3)))
    items[6] = no_lm                                                    # keypoints but no local map point
    assert len({(len(i["lm_mp"]), len(i["kp_mp"])) for i in items}) == 11
    got = LC.loop_match_to_map_batch(gpu_ctx, P, items)
    assert len(got) == 11
    for b, item in enumerate(items):
        single = LC.loop_match_to_map(gpu_ctx, P, item)
        for f in FIELDS:
            assert np.asarray(got[b][f]).tobytes() == np.asarray(single[f]).tobytes(), (b, f)
        assert got[b]["n_matches"] == single["n_matches"]
        _check(got[b], R.flat(P, item))
    assert len(got[4]["lm_status"]) == 0 and got[4]["n_matches"] == 0
    assert got[9]["n_matches"] == 0 and (got[9]["lm_kp"] == -1).all() and len(got[9]["lm_kp"]) > 0
    assert got[6]["n_matches"] == 0 and (got[6]["kp_lm"] == -1).all() and len(got[6]["kp_lm"]) > 0
    assert LC.loop_match_to_map_batch(gpu_ctx, P, []) == []


def test_euroc_sized_candidate_and_identical_repeats(gpu_ctx):
    """3080 local map points x 308 keypoints, map points of up to 80 observers (the chunked search), three times identical bytes"""
    P = R.make_params(D=R.RADTAN4)
    M = R.make_scene(P, np.random.default_rng(3080), n_kp=308, n_lm=3600, many_obs=40, dup=0.7)
    item, meta = R.flatten(M)
    assert len(item["lm_mp"]) >= 3080 and int(np.diff(item["obs_start"]).max()) > 64
    item, meta = R.trim(item, meta, 3080)
    ref = R.flat(P, item)
    runs = [LC.loop_match_to_map(gpu_ctx, P, item) for _ in range(3)]
    _check(runs[0], ref)
    for other in runs[1:]:
        for f in FIELDS:
            assert np.asarray(runs[0][f]).tobytes() == np.asarray(other[f]).tobytes(), f
    assert ref["n_matches"] > 20


@pytest.mark.parametrize("seed", [0, 1])
def test_fisheye_projection_within_one_ulp_everything_else_exact(gpu_ctx, seed):
    """atan on the device may differ from the host's in the last bit: 1 float ulp on lm_projpx, everything else exact, on scenes
    whose gate quantities all lie at least 1e-3 px from their thresholds in the reference form (the generator resamples)"""
    P = R.make_params(D=R.FISHEYE4, model="fisheye")
    M, item, meta, ref = R.filtered_scene(P, seed, min_margin=1e-3, n_kp=120, n_lm=340)
    got = LC.loop_match_to_map(gpu_ctx, P, item)
    _check(got, ref, ulp=1)
    assert ref["n_matches"] > 5


def test_invalid_arguments_leave_the_outputs(gpu_ctx):
    P = R.make_params()
    item = R.flatten(R.make_scene(P, np.random.default_rng(2), n_kp=40, n_lm=80))[0]
    s, keep, n_lm, n_kp = LC._loopmap_item(item)
    r, out = LC._loopmap_result(n_lm, n_kp)
    p = LC._as_loopmap_params(P)
    lib = gpu_ctx.lib
    assert lib.ov2_loop_match_to_map(gpu_ctx.h, C.byref(p), C.byref(s), C.byref(r)) == L.OV2_OK
    before = {f: out[f].copy() for f in FIELDS}
    for f in FIELDS:
        out[f].view(np.uint8)[...] = 0xEE
    bad = dict(item); bad["lm_mp"] = item["lm_mp"].copy(); bad["lm_mp"][0] = len(item["obs_start"]) - 1
    s2, keep2, _, _ = LC._loopmap_item(bad)
    assert lib.ov2_loop_match_to_map(gpu_ctx.h, C.byref(p), C.byref(s2), C.byref(r)) == L.OV2_EINVAL
    assert lib.ov2_loop_match_to_map(None, C.byref(p), C.byref(s), C.byref(r)) == L.OV2_EINVAL
    assert lib.ov2_loop_match_to_map_batch(gpu_ctx.h, C.byref(p), 70000, C.byref(s), C.byref(r)) == L.OV2_EUNSUPPORTED
    assert all((out[f].view(np.uint8) == 0xEE).all() for f in FIELDS), "a rejected call wrote its outputs"
    assert lib.ov2_loop_match_to_map(gpu_ctx.h, C.byref(p), C.byref(s), C.byref(r)) == L.OV2_OK
    for f in FIELDS:
        assert out[f].tobytes() == before[f].tobytes(), f


def _wr(f, a):
    a = np.ascontiguousarray(a)
    f.write(struct.pack("<q", a.nbytes)); f.write(a.tobytes())


def _rd(f, dt):
    nb = struct.unpack("<q", f.read(8))[0]
    return np.frombuffer(f.read(nb), dt)


def test_cpp_adapter(gpu_ctx, tmp_path):
    """tests/cpp/loopmap_run.cpp: ov2::LoopCloser::trackLoopLocalMap, single and batch, leaves the vkplmids of the literal replay"""
    exe = tmp_path / "loopmap_run"
    libdir = os.path.join(ROOT, "ov2slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "loopmap_run.cpp"),
                           "-o", str(exe), "-L", libdir, "-lov2slam_hip", "-Wl,-rpath," + libdir])
    P = R.make_params(D=R.RADTAN5)
    M = R.make_scene(P, np.random.default_rng(44), n_kp=150, n_lm=300)
    item, meta = R.flatten(M)
    case, res = tmp_path / "case.bin", tmp_path / "res.bin"
    with open(case, "wb") as f:
        _wr(f, np.array([L.OV2_CAM_PINHOLE, P["ncellsize"]], np.int32))
        _wr(f, np.array([P["fmax_proj_pxdist"], P["fmax_desc_dist"]], np.float32))
        _wr(f, np.array(list(P["K"]) + [P["img_w"], P["img_h"]], np.float64))
        _wr(f, np.array(P["D"], np.float64))
        _wr(f, item["Tcw"]); _wr(f, np.array(meta["kp_lmid"], np.int32)); _wr(f, item["kp_px"]); _wr(f, item["kp_mp"]); _wr(f, item["kp_matched"])
        _wr(f, item["cell_start"]); _wr(f, item["cell_kp"]); _wr(f, item["obs_start"]); _wr(f, item["obs_kfid"])
        _wr(f, item["desc_start"]); _wr(f, item["desc"])
        _wr(f, np.array(meta["lm_lmid"], np.int32)); _wr(f, item["lm_mp"]); _wr(f, item["lm_wpt"])
        _wr(f, np.array(meta["walk_vkplmids"], np.int32).reshape(-1, 2))
    r = subprocess.run([str(exe), str(case), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    py = LC.loop_match_to_map(gpu_ctx, P, item)
    want, info = R.replay(M)
    assert len(want) > len(meta["walk_vkplmids"]) + 5 and R.vkplmids_of(py, meta) == want
    with open(res, "rb") as f:
        for form in ("single", "batch"):
            vk, kp_lm, st = _rd(f, np.int32).reshape(-1, 2), _rd(f, np.int32), _rd(f, np.uint8)
            assert np.array_equal(kp_lm, py["kp_lm"]) and np.array_equal(st, py["lm_status"]), form
            assert [(int(a), int(b)) for a, b in vk] == want, form
