"""The tracking priors on the GPU (csrc/priors.hip: ov2_klt_priors, ov2_stereo_priors and their batch forms) against the flat form
of tests/priors_ref.py over the scenes of tests/test_priors_reference.py: pinhole cameras bit for bit (prior as float bits,
has_prior and skip as bytes); the fisheye camera within one float ulp on prior -- the project's bound for atan, as for
ov2_match_to_map -- and equal flags, its scenes keeping every projection 1e-3 px away from the image edges; batches of 1, 3 (one item
empty) and 11 against the reference and against single calls, byte for byte; byte-identical repeats; the crafted cases; and the
C++ adapters (ov2slam_amd/host: ov2::kltPriors, ov2::stereoPriors) against the literal replay."""
import os
import struct
import subprocess

import numpy as np
import pytest

from ov2slam_amd import _lib as L
from ov2slam_amd import priors as PR
from tests import priors_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FORMS = {"klt": (R.flat_klt, PR.klt_priors, PR.klt_priors_batch), "stereo": (R.flat_stereo, PR.stereo_priors, PR.stereo_priors_batch)}
_CACHE = {}


def _camera_scenes(form, ci):
    """[(name, P, item, flat reference, ev)] of camera ci, computed once"""
    if (form, ci) not in _CACHE:
        model, Dv = R.CAMERAS[ci]
        out = []
        for name, P, frame, mps in R.scene_list(form):
            if (P["model"], P["D"]) != (model, None if Dv is None else tuple(Dv)):
                continue
            item = R.flatten(P, frame, mps)
            ev = {}
            out.append((name, P, item, FORMS[form][0](P, item, ev), ev))
        assert len(out) == len(R.SCENE_NS)
        _CACHE[(form, ci)] = out
    return _CACHE[(form, ci)]


def _check(got, ref, P, what):
    ok, field = R.same(ref, got, prior_ulp=1 if P["model"] == "fisheye" else 0)
    assert ok, (what, field)
    assert got["prior"].dtype == np.float32 and got["has_prior"].dtype == np.uint8
    if "skip" in ref:
        assert (got["n_prior3d"], got["n_prior_nb"], got["n_skip"]) == (int((ref["has_prior"] == 1).sum()), int((ref["has_prior"] == 2).sum()),
                                                                      int(ref["skip"].sum())), what
    else:
        assert got["n_prior"] == int(ref["has_prior"].sum()), what


def _bytes(res):
    return b"".join(np.ascontiguousarray(res[f]).tobytes() for f in ("prior", "has_prior", "skip") if f in res)


@pytest.mark.parametrize("ci", range(len(R.CAMERAS)), ids=["pinhole0", "pinhole4", "pinhole8", "fisheye4"])
@pytest.mark.parametrize("form", ["klt", "stereo"])
def test_single_calls_against_the_flat_reference(gpu_ctx, form, ci):
    for name, P, item, ref, ev in _camera_scenes(form, ci):
        if P["model"] == "fisheye":
            assert ev.get("margin", np.inf) >= 1e-3, (name, ev)     # the property the flag comparison rests on
        _check(FORMS[form][1](gpu_ctx, P, item), ref, P, name)


@pytest.mark.parametrize("ci", range(len(R.CAMERAS)), ids=["pinhole0", "pinhole4", "pinhole8", "fisheye4"])
@pytest.mark.parametrize("form", ["klt", "stereo"])
def test_batches_against_the_reference_and_single_calls(gpu_ctx, form, ci):
    flat, single, batch = FORMS[form]
    scenes = _camera_scenes(form, ci)
    by_n = {len(s[2]["px"]): s for s in scenes}
    P = dict(by_n[308][1], klt_use_prior=True, rect=False)           # one params struct for the whole batch
    order = [308, 0, 63, 1, 130, 64, 2, 65, 130, 63, 308]
    for ns in ([308], [130, 0, 65], order):
        items = [by_n[n][2] for n in ns]
        evs = [dict() for _ in items]
        refs = [flat(P, it, ev) for it, ev in zip(items, evs)]
        if P["model"] == "fisheye":
            assert all(ev.get("margin", np.inf) >= 1e-3 for ev in evs)
        got = batch(gpu_ctx, P, items)
        assert len(got) == len(ns)
        for b, (g, r) in enumerate(zip(got, refs)):
            _check(g, r, P, (ns, b))
            assert _bytes(g) == _bytes(single(gpu_ctx, P, items[b])), (ns, b)      # every batch item equals its single call
        again = batch(gpu_ctx, P, items)
        assert [_bytes(g) for g in got] == [_bytes(g) for g in again]           # two runs give the same bytes
    assert batch(gpu_ctx, P, []) == []


def test_crafted_cases(gpu_ctx):
    for name, P, frame, mps, exp in R.crafted_klt():
        item = R.flatten(P, frame, mps)
        got = PR.klt_priors(gpu_ctx, P, item)
        _check(got, R.flat_klt(P, item), P, name)
        assert got["has_prior"].tolist() == exp, name
    cases = R.crafted_stereo()
    for name, P, frame, mps, exp, skip in cases:
        item = R.flatten(P, frame, mps)
        got = PR.stereo_priors(gpu_ctx, P, item)
        _check(got, R.flat_stereo(P, item), P, name)
        assert got["has_prior"].tolist() == exp and got["skip"].tolist() == skip, name
    # and all of one params struct in one batch
    P0 = cases[0][1]
    same_p = [c for c in cases if c[1] == P0]
    items = [R.flatten(P0, c[2], c[3]) for c in same_p]
    for c, g in zip(same_p, PR.stereo_priors_batch(gpu_ctx, P0, items)):
        assert g["has_prior"].tolist() == c[4] and g["skip"].tolist() == c[5], c[0]


def test_stereo_priors_feed_stereo_match_unchanged(gpu_ctx):
    """the stereo form's outputs have the layout ov2_stereo_match takes: (n, 2) float32 priors and a byte per keypoint, non-zero =
    a prior of either kind"""
    name, P, item, ref, ev = _camera_scenes("stereo", 1)[-1]
    got = PR.stereo_priors(gpu_ctx, P, item)
    assert got["prior"].shape == (308, 2) and got["prior"].flags["C_CONTIGUOUS"] and got["has_prior"].shape == (308,)
    assert set(np.unique(got["has_prior"])) <= {0, 1, 2} and np.array_equal(got["has_prior"] != 0, ref["has_prior"] != 0)


def _wr(f, a):
    a = np.ascontiguousarray(a)
    f.write(struct.pack("<q", a.nbytes)); f.write(a.tobytes())


def _rd(f, dt):
    nb = struct.unpack("<q", f.read(8))[0]
    return np.frombuffer(f.read(nb), dt)


def test_cpp_adapters(gpu_ctx, tmp_path):
    """tests/cpp/priors_run.cpp: ov2::kltPriors / ov2::stereoPriors, single and batch, on keypoints handed over in the map's order
    with the grid as per-cell lists (the adapter builds the offsets), against the literal replay of the reference's loops"""
    exe = tmp_path / "priors_run"
    libdir = os.path.join(ROOT, "ov2slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "priors_run.cpp"),
                           "-o", str(exe), "-L", libdir, "-lov2slam_hip", "-Wl,-rpath," + libdir])
    P = R.make_params(D=R.RADTAN8, klt_use_prior=True, rect=False)
    scenes = [R.make_scene(P, np.random.default_rng(80 + k), n, pgone=0.0 if k == 0 else 0.15) for k, n in enumerate((308, 65, 0))]
    case, res = tmp_path / "case.bin", tmp_path / "res.bin"
    with open(case, "wb") as f:
        _wr(f, np.array([L.OV2_CAM_PINHOLE, P["ncellsize"], int(P["rect"]), int(P["klt_use_prior"]), len(scenes)], np.int32))
        _wr(f, np.array(list(P["K"]) + [P["img_w"], P["img_h"]] + list(P["Tcic0"]), np.float64))
        _wr(f, np.array(P["D"], np.float64))
        for frame, mps in scenes:
            it = R.flatten(P, frame, mps)
            for name in ("px", "unpx", "bv", "wpt", "state"):
                _wr(f, it[name])
            _wr(f, (it["state"] == 1).astype(np.uint8))            # the frame form: 3-D = with its map point (map_plms_.at())
            _wr(f, it["Tcw"]); _wr(f, it["cell_start"]); _wr(f, it["cell_kp"])
    subprocess.run([str(exe), str(case), str(res)], check=True, timeout=120)
    with open(res, "rb") as f:
        for rnd in ("single", "batch"):
            for frame, mps in scenes:
                n = len(frame["mapkps_"])
                kframe = dict(frame, mapkps_={i: dict(k, is3d=k["is3d"] and i in mps) for i, k in frame["mapkps_"].items()})
                kref = R.klt_arrays(kframe, R.replay_klt(P, kframe, mps))
                sref = R.stereo_arrays(frame, R.replay_stereo(P, frame, mps))
                kgot = dict(prior=_rd(f, np.float32).reshape(n, 2), has_prior=_rd(f, np.uint8))
                sgot = dict(prior=_rd(f, np.float32).reshape(n, 2), has_prior=_rd(f, np.uint8), skip=_rd(f, np.uint8))
                assert R.same(kref, kgot)[0] and R.same(sref, sgot)[0], (rnd, n)
        assert f.read() == b""
