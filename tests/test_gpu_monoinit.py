"""The device mono initialisation chain (csrc/monoinit.hip, ov2_mono_init[_batch]) on the GPU against the numpy specification
(tests/monoinit_ref.py) on every named scene.  The bound is the project's standard for the searches where no fragile row is consumed
(tests/test_monoinit_reference.py asserts that of the scenes): every integer and byte of the result equals the specification, every
float and double equals it bit for bit, and the table the device drew is ov2_epipolar_draw_samples'.  The decisions (everything that
is an integer, a byte or one of the two float parallaxes) and the numbers (model, Twc_init) are asserted in two tests, so that a
last-bit difference of the search's model could not hide a wrong decision.  Then p0 against ov2_parallax itself, the batch form
(whole, in halves, reversed) against the single call, and two runs against each other."""
import numpy as np
import pytest

from tests import kfreq_ref as KF
from tests import monoinit_ref as R

INT_FIELDS = ("action", "nb2dkps", "p0_n", "p0_n_distinct", "p0_n_nonfinite", "m", "status", "best_row", "iterations", "rows_consumed",
              "n_inliers", "n_outliers", "n_removed", "pose_refined")
F32_FIELDS = ("p0", "p1")
F64_FIELDS = ("model", "Twc_init")

_got = {}


def _run(ctx, name):
    """the chain's result on a named scene (one single call per scene and session, with the table traced)"""
    from ov2slam_amd import keyframe
    if name not in _got:
        P, cur, kf = R.scene(name)
        _got[name] = keyframe.mono_init(ctx, P, R.flatten(cur, kf), trace_samples=True)
    return _got[name]


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_bytes(a, b, what=""):
    """two result dicts of the chain, byte for byte"""
    for k in INT_FIELDS:
        assert int(a[k]) == int(b[k]), (what, k)
    for k in F32_FIELDS:
        assert KF.bits(a[k]) == KF.bits(b[k]), (what, k)
    for k in F64_FIELDS + ("score",):
        assert np.array_equal(_bits64(a[k]), _bits64(b[k])), (what, k)
    assert np.array_equal(a["removed"], b["removed"]) and np.array_equal(a["pair_cur"], b["pair_cur"]), what
    if a.get("samples") is None or b.get("samples") is None:
        assert a.get("samples") is None and b.get("samples") is None, what
    else:
        assert np.array_equal(a["samples"], b["samples"]), what


@pytest.mark.gpu
@pytest.mark.parametrize("name", R.SCENE_NAMES)
def test_decisions_equal_the_specification(gpu_ctx, name):
    from ov2slam_amd import pose
    P, cur, kf = R.scene(name)
    got, want = _run(gpu_ctx, name), R.expected(name)
    print("%s: %s, nb2dkps %d, p0 %r, m %d, p1 %r, status %d, inliers %d, removed %d" % (
        name, R.ACTIONS.get(got["action"], got["action"]), got["nb2dkps"], got["p0"], got["m"], got["p1"], got["status"], got["n_inliers"],
        got["n_removed"]))
    for k in INT_FIELDS:
        assert int(got[k]) == int(want[k]), (k, got[k], want[k])
    for k in F32_FIELDS:
        assert KF.bits(got[k]) == KF.bits(want[k]), (k, got[k], want[k])
    assert float(got["score"]) == float(want["score"])
    assert np.array_equal(got["removed"], want["removed"])
    assert np.array_equal(got["pair_cur"], want["pair_cur"])
    if want["samples"] is None or P["n_rows"] == 0:
        assert got["samples"] is None
    else:
        assert np.array_equal(got["samples"], want["samples"])
        assert np.array_equal(got["samples"], pose.epipolar_draw_samples(int(cur["seed"]), got["m"], P["n_rows"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", R.SCENE_NAMES)
def test_numbers_equal_the_specification_bit_for_bit(gpu_ctx, name):
    got, want = _run(gpu_ctx, name), R.expected(name)
    print("%s: largest |device - specification| over model / Twc_init %.3g" % (
        name, max(float(np.abs(got[k] - want[k]).max()) for k in F64_FIELDS)))
    for k in F64_FIELDS:
        assert np.array_equal(_bits64(got[k]), _bits64(want[k])), k


@pytest.mark.gpu
@pytest.mark.parametrize("name", R.SCENE_NAMES)
def test_pose_follows_from_the_device_model_and_p0_is_ov2_parallax(gpu_ctx, name):
    """Twc_init is the specification's restatement applied to the model the DEVICE found, bit for bit; p0 is what the separate call
    returns for the same item"""
    from ov2slam_amd import keyframe
    P, cur, kf = R.scene(name)
    got = _run(gpu_ctx, name)
    if got["action"] == R.READY:
        assert np.array_equal(_bits64(got["Twc_init"]), _bits64(R.init_pose(got["model"])))
    else:
        assert not got["Twc_init"].any() and not got["removed"].any() and got["n_removed"] == 0
    if got["action"] != R.RESET:
        p = keyframe.parallax(gpu_ctx, P["fkf"], R.flatten(cur, kf), unrot=0, filter=keyframe.ALL, stat=keyframe.MEDIAN)
        assert (KF.bits(p["parallax"]), p["n"], p["n_distinct"], p["n_nonfinite"]) == \
               (KF.bits(got["p0"]), got["p0_n"], got["p0_n_distinct"], got["p0_n_nonfinite"])


def _groups():
    """the scenes by their params (a batch shares them), largest group first"""
    by = {}
    for n in R.SCENE_NAMES:
        P = R.scene(n)[0]
        key = (P["n_rows"], P["min_2d_kps"], P["fkf"]["K"], P["fkf"]["finit_parallax"])
        by.setdefault(key, []).append(n)
    return sorted(by.values(), key=len, reverse=True)


@pytest.mark.gpu
def test_batch_items_equal_the_single_call(gpu_ctx):
    """every scene as an item of a batch with the scenes that share its params -- whole, in two halves and reversed -- and, so that
    every scene meets items of other sizes and actions, all of them once more in one batch with the rows of the largest table"""
    from ov2slam_amd import keyframe
    for names in _groups():
        P = R.scene(names[0])[0]
        items = [R.flatten(*R.scene(n)[1:]) for n in names]
        whole = keyframe.mono_init_batch(gpu_ctx, P, items, trace_samples=True)
        h = len(items) // 2
        halves = keyframe.mono_init_batch(gpu_ctx, P, items[:h], trace_samples=True) + \
            keyframe.mono_init_batch(gpu_ctx, P, items[h:], trace_samples=True)
        rev = keyframe.mono_init_batch(gpu_ctx, P, items[::-1], trace_samples=True)[::-1]
        for n, a, b, c in zip(names, whole, halves, rev):
            single = _run(gpu_ctx, n)
            _same_bytes(a, single, n + " whole")
            _same_bytes(b, single, n + " halves")
            _same_bytes(c, single, n + " reversed")
    names = [n for n in R.SCENE_NAMES if R.scene(n)[0]["fkf"]["K"] == KF.EUROC_K and R.scene(n)[0]["min_2d_kps"] == 0]
    P = dict(R.scene(names[0])[0], n_rows=200)
    items = [R.flatten(*R.scene(n)[1:]) for n in names]
    mixed = keyframe.mono_init_batch(gpu_ctx, P, items, trace_samples=True)
    for n, it, a in zip(names, items, mixed):
        _same_bytes(a, keyframe.mono_init(gpu_ctx, P, it, trace_samples=True), n + " mixed")
    assert {a["action"] for a in mixed} >= {R.LOW_PARALLAX, R.TOO_FEW_KPS, R.TOO_FEW_MATCHES, R.LOW_ROT_PARALLAX, R.NO_MODEL, R.READY}


@pytest.mark.gpu
def test_two_runs_give_equal_bytes(gpu_ctx):
    from ov2slam_amd import keyframe
    names = ("size_308_rows_200", "outliers_over_half", "quat_x", "n_kf_0")
    P = dict(R.scene(names[0])[0], n_rows=200)
    items = [R.flatten(*R.scene(n)[1:]) for n in names]
    a = keyframe.mono_init_batch(gpu_ctx, P, items, trace_samples=True)
    b = keyframe.mono_init_batch(gpu_ctx, P, items, trace_samples=True)
    for n, x, y in zip(names, a, b):
        _same_bytes(x, y, n)


@pytest.mark.gpu
def test_empty_frames_and_an_empty_batch(gpu_ctx):
    from ov2slam_amd import keyframe
    from tests import epifilter_ref as EF
    P = R.make_P(n_rows=16)
    cur, kf = EF.geo_scene(71, 0, extra_kf=0)
    r = keyframe.mono_init(gpu_ctx, P, R.flatten(cur, kf))
    assert (r["action"], r["nb2dkps"], r["p0_n"], float(r["p0"]), r["m"]) == (R.LOW_PARALLAX, 0, 0, 0.0, 0) and len(r["removed"]) == 0
    r = keyframe.mono_init(gpu_ctx, dict(P, min_2d_kps=1), R.flatten(cur, kf))
    assert r["action"] == R.RESET
    assert keyframe.mono_init_batch(gpu_ctx, P, []) == []
