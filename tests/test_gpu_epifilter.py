"""The device epipolar2d2dFiltering chain (csrc/epifilter.hip, ov2_epipolar_filter[_batch]) on the GPU:
  - against the numpy specification (tests/epifilter_ref.py) on every named scene.  The bound is the project's standard for the
    searches where no fragile row is consumed (tests/test_epifilter_reference.py asserts that of the scenes): every integer, byte
    and float / double bit of the result equals the specification.  The decisions (everything that is an integer, a byte or the
    float parallax) and the numbers (model, F, Twc_model, err) are asserted in two tests, so that a last-bit difference of the
    search's model could not hide a wrong decision;
  - against the route of separate calls (ov2_parallax(AVG_WIDE), a host join, ov2_epipolar_draw_samples, ov2_epipolar_ransac, F of
    the specification from that model, ov2_sampson_filter_2d), byte for byte: this pins the chain to device code that is already
    pinned, independently of the new numpy;
  - the table the device draws against ov2_epipolar_draw_samples; the batch form; the C++ adapter; planted mismatches through real
    tracker bearings."""
import os
import subprocess

import numpy as np
import pytest

from tests import epifilter_ref as R
from tests import fivept_ref as E5
from tests import kfreq_ref as KF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_FIELDS = ("action", "m", "epifrom3dkps", "do_optimize", "nb3dkps", "status", "best_row", "iterations", "rows_consumed",
              "n_inliers", "n_outliers", "n_removed_ransac", "n_removed_sampson", "pose_from_model")
F64_FIELDS = ("model", "F", "Twc_model")


def _params(P):
    return dict(fkf=P["fkf"], max_iterations=P["max_iterations"], threshold=P["threshold"], probability=P["probability"],
                fransac_err=P["fransac_err"], mono=P["mono"], n_rows=P["n_rows"])


_got = {}


def _run(ctx, name):
    """the chain's result on a named scene (one call per scene and session, with the table traced)"""
    from ov2slam_amd import keyframe
    if name not in _got:
        P, cur, kf = R.scene(name)
        _got[name] = keyframe.epipolar_filter(ctx, _params(P), R.flatten(cur, kf), trace_samples=True)
    return _got[name]


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_bytes(a, b):
    """two result dicts of the chain, byte for byte (a NaN parallax equals a NaN parallax)"""
    for k in INT_FIELDS:
        assert int(a[k]) == int(b[k]), k
    assert KF.bits(a["parallax"]) == KF.bits(b["parallax"])
    for k in F64_FIELDS + ("score",):
        assert np.array_equal(_bits64(a[k]), _bits64(b[k])), k
    assert np.array_equal(a["removed"], b["removed"]) and np.array_equal(a["pair_cur"], b["pair_cur"])
    assert np.array_equal(a["err"].view(np.uint32), b["err"].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", R.SCENE_NAMES)
def test_decisions_equal_the_specification(gpu_ctx, name):
    got, want = _run(gpu_ctx, name), R.expected(name)
    for k in INT_FIELDS:
        assert int(got[k]) == int(want[k]), (k, got[k], want[k])
    assert KF.bits(got["parallax"]) == KF.bits(want["parallax"])
    assert float(got["score"]) == float(want["score"])
    assert np.array_equal(got["removed"], want["removed"])
    assert np.array_equal(got["pair_cur"], want["pair_cur"])
    if want["samples"] is None:
        assert got["samples"] is None
    else:
        assert np.array_equal(got["samples"], want["samples"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", R.SCENE_NAMES)
def test_numbers_equal_the_specification_bit_for_bit(gpu_ctx, name):
    got, want = _run(gpu_ctx, name), R.expected(name)
    worst = max(float(np.abs(got[k] - want[k]).max()) for k in F64_FIELDS)
    print("%s: largest |device - specification| over model / F / Twc_model %.3g, err %.3g" % (
        name, worst, float(np.abs(got["err"].astype(np.float64) - want["err"]).max()) if len(want["err"]) else 0.0))
    for k in F64_FIELDS:
        assert np.array_equal(_bits64(got[k]), _bits64(want[k])), k
    assert np.array_equal(got["err"].view(np.uint32), want["err"].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", R.SCENE_NAMES)
def test_numbers_follow_from_the_device_model(gpu_ctx, name):
    """F, the mono pose and the Sampson errors are the specification's restatements applied to the model the DEVICE found, bit for
    bit: whatever the search's last bits are, everything behind it is exact"""
    P, cur, kf = R.scene(name)
    got = _run(gpu_ctx, name)
    if got["pose_from_model"]:
        assert np.array_equal(_bits64(got["Twc_model"]), _bits64(R.mono_pose(kf["Twc"], kf["Tcw"], cur["Twc"], got["model"])))
    else:
        assert not got["Twc_model"].any()
    if got["action"] == R.FILTERED and got["epifrom3dkps"]:
        F = R.fundamental(P["fkf"]["K"], got["model"])
        assert np.array_equal(_bits64(got["F"]), _bits64(F))
        err, bad, n_bad = KF.flat_sampson(R.flatten(cur, kf), F, P["fransac_err"])
        assert np.array_equal(got["err"].view(np.uint32), err.view(np.uint32))
        assert np.array_equal(got["removed"] == 2, bad != 0) and got["n_removed_sampson"] == n_bad
    else:
        assert not got["F"].any() and not got["err"].any() and got["n_removed_sampson"] == 0


def _route(ctx, P, item):
    """the route of separate calls: three device calls, three synchronisations, the join, the draw and F on the host"""
    from ov2slam_amd import keyframe, pose
    n = len(item["cur_lmid"])
    nb3d = int(item.get("nb3dkps", -1))
    if nb3d < 0:
        nb3d = int((item["cur_is3d"] != 0).sum())
    from3d = bool(P["fkf"]["stereo"]) and nb3d > 30
    par = keyframe.parallax(ctx, P["fkf"], item, unrot=1, filter=keyframe.ONLY_3D if from3d else keyframe.ALL, stat=keyframe.AVG_WIDE)
    j = np.searchsorted(item["kf_lmid"], item["cur_lmid"])
    hit = (j < len(item["kf_lmid"])) & (item["kf_lmid"][np.minimum(j, max(len(item["kf_lmid"]) - 1, 0))] == item["cur_lmid"]) \
        if len(item["kf_lmid"]) else np.zeros(n, bool)
    if from3d:
        hit = hit & (item["cur_is3d"] != 0)
    pair_cur = np.nonzero(hit)[0].astype(np.int32)
    r = dict(parallax=par["parallax"], m=len(pair_cur), pair_cur=pair_cur, removed=np.zeros(n, np.uint8), err=np.zeros(n, np.float32),
             F=np.zeros(9), model=np.zeros(12), search=None, epifrom3dkps=int(from3d), nb3dkps=nb3d, action=R.NO_MODEL)
    assert par["n"] == r["m"]
    if n < 8:
        r["action"] = R.TOO_FEW_KPS
        return r
    if np.float64(par["parallax"]) < 2.0 * np.float64(np.float32(P["fransac_err"])):
        r["action"] = R.LOW_PARALLAX
        return r
    m = r["m"]
    sm = pose.epipolar_draw_samples(item["seed"], m, P["n_rows"]) if m >= 8 else np.zeros((0, 8), np.int32)
    s = pose.epipolar_ransac(ctx, pose.epipolar_params(P["max_iterations"], P["threshold"], P["probability"]),
                             dict(bv1=item["kf_bv"][j[pair_cur]], bv2=item["cur_bv"][pair_cur], samples=sm))
    r.update(search=s, model=s["model"], samples=sm)
    if s["status"] != 0:
        return r
    if float(len(s["outliers"])) > 0.5 * float(m):
        r["action"] = R.DEGENERATE
        return r
    r["action"] = R.FILTERED
    r["removed"][pair_cur[s["outliers"]]] = 1
    if from3d:
        r["F"] = R.fundamental(P["fkf"]["K"], s["model"])
        sp = keyframe.sampson_filter_2d(ctx, item, r["F"], P["fransac_err"])
        r["err"] = sp["err"]
        r["removed"][sp["bad"] != 0] = 2
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("name", R.SCENE_NAMES)
def test_chain_equals_the_route_of_separate_calls(gpu_ctx, name):
    P, cur, kf = R.scene(name)
    got, want = _run(gpu_ctx, name), _route(gpu_ctx, P, R.flatten(cur, kf))
    for k in ("action", "m", "epifrom3dkps", "nb3dkps"):
        assert int(got[k]) == int(want[k]), k
    assert KF.bits(got["parallax"]) == KF.bits(want["parallax"])
    assert np.array_equal(got["pair_cur"], want["pair_cur"])
    assert np.array_equal(got["removed"], want["removed"])
    assert np.array_equal(got["err"].view(np.uint32), want["err"].view(np.uint32))
    assert np.array_equal(_bits64(got["F"]), _bits64(want["F"]))
    s = want["search"]
    if s is None:
        assert (got["status"], got["best_row"], got["iterations"], got["rows_consumed"]) == (0, -1, 0, 0) and not got["model"].any()
        return
    assert np.array_equal(_bits64(got["model"]), _bits64(s["model"]))
    assert (got["status"], got["best_row"], got["iterations"], got["rows_consumed"], got["n_inliers"], got["n_outliers"]) == \
           (s["status"], s["best_row"], s["iterations"], s["rows_consumed"], s["n_inliers"], len(s["outliers"]))
    assert float(got["score"]) == float(s["score"])


def _table_item(m, seed):
    """m joined keypoints far above the gate (exact_scene: identity poses, K = (1, 1, 0, 0), parallax = the integer given)"""
    rng = np.random.default_rng(m)
    cur, kf = KF.exact_scene([float(v) for v in rng.integers(8, 40, m)])
    for k in kf["kps"].values():
        k["bv"] = (0., 0., 1.)
    kf["Twc"] = np.array(KF._ID7)
    cur.update(nbkfs=3, seed=seed)
    return R.flatten(cur, kf)


@pytest.mark.gpu
@pytest.mark.parametrize("n_rows", (1, 64, 65, 200))
def test_device_drawn_table_equals_draw_samples(gpu_ctx, n_rows):
    from ov2slam_amd import keyframe, pose
    P = R.make_P(n_rows=n_rows, max_iterations=1)
    P["fkf"] = KF._unit_params()
    ms = (8, 9, 64, 215, 2048)
    items = [_table_item(m, 77 * m + n_rows) for m in ms]
    out = keyframe.epipolar_filter_batch(gpu_ctx, _params(P), items, trace_samples=True)
    for m, it, o in zip(ms, items, out):
        assert o["m"] == m and o["action"] >= R.NO_MODEL
        want = pose.epipolar_draw_samples(it["seed"], m, n_rows)
        assert np.array_equal(o["samples"], want), (m, n_rows)
        if m <= 64:
            assert np.array_equal(want, E5.draw_samples(it["seed"], m, n_rows))
        assert all(len(set(r)) == 8 for r in o["samples"].tolist())


def _draws_per_row(seed, m, rows):
    """how many draws of the stream each row of fivept_ref.draw_samples(seed, m, rows) consumes"""
    out, j = [], 0
    for _ in range(rows):
        seen, c = set(), 0
        while len(seen) < 8:
            seen.add(E5._splitmix64(seed & ((1 << 64) - 1), j) % m)
            j += 1
            c += 1
        out.append(c)
    return out


# (n_rows, seed) at m = 8 whose LAST row consumes more draws than the short window the kernel first tries for the rows that are left
# (16 per row + 64): 85 and 100 draws for a table of one row; 96 and 101 behind a first row of 26 / 28; 118 behind eight rows of 181
LONG_LAST_ROWS = ((1, 8601), (1, 12017), (2, 6999), (2, 13456), (9, 11188))


@pytest.mark.gpu
@pytest.mark.parametrize("n_rows,seed", LONG_LAST_ROWS)
def test_a_row_longer_than_the_short_window_is_drawn_like_the_host(gpu_ctx, n_rows, seed):
    from ov2slam_amd import keyframe, pose
    per_row = _draws_per_row(seed, 8, n_rows)
    assert per_row[-1] > 16 * 1 + 64 and sum(per_row[:-1]) + per_row[-1] > 16 * n_rows + 64, per_row
    P = R.make_P(n_rows=n_rows, max_iterations=5)
    P["fkf"] = KF._unit_params()
    item = _table_item(8, seed)
    got = keyframe.epipolar_filter(gpu_ctx, _params(P), item, trace_samples=True)
    want = pose.epipolar_draw_samples(seed, 8, n_rows)
    assert got["m"] == 8 and np.array_equal(got["samples"], want) and np.array_equal(want, E5.draw_samples(seed, 8, n_rows))
    s = pose.epipolar_ransac(gpu_ctx, pose.epipolar_params(5, P["threshold"]), dict(bv1=item["kf_bv"], bv2=item["cur_bv"], samples=want))
    assert (got["status"], got["best_row"], got["iterations"], got["rows_consumed"], got["n_inliers"]) == \
           (s["status"], s["best_row"], s["iterations"], s["rows_consumed"], s["n_inliers"])
    assert np.array_equal(_bits64(got["model"]), _bits64(s["model"]))


def _batch_items():
    """70 items of mixed sizes under ONE parameter set, empty ones and every action among them; item 0, 3 and 69 are the same"""
    P = R.make_P(mono=True, n_rows=200)
    names = ("outliers_half_plus_1", "n_cur_7", "m_7_of_12", "size_64_rows_64", "mono_quat_x", "outliers_half", "size_308_rows_200",
             "m_0_nan_parallax", "n_kf_0", "inliers_9", "inliers_10", "mono_nbkfs_3_nb3d_29", "size_65_rows_65", "m_8_of_12")
    pool = [R.flatten(*R.scene(n)[1:]) for n in names]
    pool.append(R.flatten(*R.geo_scene(70, 20, rel_t=(0.001, 0.0, 0.0))))            # no parallax
    empty = R.flatten(*R.geo_scene(71, 0, extra_kf=0))
    pool.append(empty)
    pool.append(R.flatten(*R.geo_scene(72, 0, extra_kf=9)))                            # an empty frame against a keyframe
    same = R.flatten(*R.scene("mono_quat_y")[1:])
    items = [pool[b % len(pool)] for b in range(70)]
    items[0] = items[3] = items[69] = same
    return P, items


@pytest.mark.gpu
def test_batch_equals_single_calls_at_every_position_and_twice(gpu_ctx):
    from ov2slam_amd import keyframe
    P, items = _batch_items()
    a = keyframe.epipolar_filter_batch(gpu_ctx, _params(P), items)
    b = keyframe.epipolar_filter_batch(gpu_ctx, _params(P), items)
    assert {o["action"] for o in a} == {R.TOO_FEW_KPS, R.LOW_PARALLAX, R.NO_MODEL, R.DEGENERATE, R.FILTERED}
    assert any(len(o["removed"]) == 0 for o in a)
    single = {}
    for i, (it, oa, ob) in enumerate(zip(items, a, b)):
        _same_bytes(oa, ob)
        if id(it) not in single:
            single[id(it)] = keyframe.epipolar_filter(gpu_ctx, _params(P), it)
        _same_bytes(oa, single[id(it)])
    _same_bytes(a[0], a[3])
    _same_bytes(a[0], a[69])
    assert a[0]["action"] == R.FILTERED and a[0]["pose_from_model"] == 1


@pytest.mark.gpu
def test_capacity_layout_block_equals_the_packed_one(gpu_ctx):
    """epif_chain_enqueue on a block at CAPACITY layout (every item owns the slots of the largest item and n_rows rows: what a fused
    step will hand it), forced through OV2_OPT_EPIF_CAPACITY, against the block packed to the items' sizes: byte for byte, the table
    included"""
    from ov2slam_amd import keyframe
    from ov2slam_amd import _lib as L
    P, items = _batch_items()
    items = items[:24]                                                         # 0 to 308 keypoints, empty ones, every action
    a = keyframe.epipolar_filter_batch(gpu_ctx, _params(P), items, trace_samples=True)
    gpu_ctx.set_option(L.OV2_OPT_EPIF_CAPACITY, 1)
    try:
        b = keyframe.epipolar_filter_batch(gpu_ctx, _params(P), items, trace_samples=True)
        one = keyframe.epipolar_filter(gpu_ctx, _params(P), items[6])
    finally:
        gpu_ctx.set_option(L.OV2_OPT_EPIF_CAPACITY, 0)
    assert {o["action"] for o in a} == {R.TOO_FEW_KPS, R.LOW_PARALLAX, R.NO_MODEL, R.DEGENERATE, R.FILTERED}
    assert len({len(o["removed"]) for o in a}) > 6
    for oa, ob in zip(a, b):
        _same_bytes(oa, ob)
        assert (oa["samples"] is None) == (ob["samples"] is None) and (oa["samples"] is None or np.array_equal(oa["samples"], ob["samples"]))
    _same_bytes(a[6], one)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """tests/cpp/epifilter_run.cpp, compiled once per session against the built library"""
    exe = tmp_path_factory.mktemp("epifilter") / "epifilter_run"
    libdir = os.path.join(ROOT, "ov2slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "epifilter_run.cpp"),
                           "-o", str(exe), "-L", libdir, "-lov2slam_hip", "-Wl,-rpath," + libdir])
    return str(exe)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("stereo_2d_unknown_to_keyframe", "size_64_rows_64", "outliers_half_plus_1", "mono_quat_z", "m_7_of_12"))
def test_cpp_adapter_returns_the_specifications_lmids(gpu_ctx, driver, name, tmp_path):
    """ov2::epipolar2d2dFiltering (host/visual_front_end.hpp) with the keyframe side SHUFFLED: the lmids to remove, in the
    reference's order"""
    P, cur, kf = R.scene(name)
    want = R.expected(name)
    item = R.flatten(cur, kf)
    perm = np.random.default_rng(3).permutation(len(item["kf_lmid"]))
    path = tmp_path / "in.txt"
    with open(path, "w") as f:
        K = P["fkf"]["K"]
        f.write("%r %r %r %r %d %d %d %r %r %r %d\n" % (K[0], K[1], K[2], K[3], int(P["fkf"]["stereo"]), int(P["mono"]), P["max_iterations"],
                                                        P["threshold"], P["probability"], P["fransac_err"], P["n_rows"]))
        f.write("%d %d %d %d %d\n" % (len(item["cur_lmid"]), len(perm), item["nbkfs"], item["seed"], item["nb3dkps"]))
        for name7 in ("cur_Twc", "kf_Tcw", "kf_Twc"):
            f.write(" ".join(repr(float(v)) for v in item[name7]) + "\n")
        for i in range(len(item["cur_lmid"])):
            f.write("%d %d %r %r %r %r %r %r %r\n" % ((item["cur_lmid"][i], item["cur_is3d"][i]) + tuple(float(v) for v in item["cur_px"][i])
                                                      + tuple(float(v) for v in item["cur_unpx"][i]) + tuple(float(v) for v in item["cur_bv"][i])))
        for j in perm:
            f.write("%d %r %r %r %r %r\n" % ((item["kf_lmid"][j],) + tuple(float(v) for v in item["kf_unpx"][j])
                                             + tuple(float(v) for v in item["kf_bv"][j])))
    out = subprocess.run([driver, str(path)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split("\n")
    head = [int(v) for v in lines[0].split()]
    assert head[0] == want["action"] and head[1] == want["m"]
    assert [int(v) for v in lines[1].split()] == R.remove_lmids(cur, want)


@pytest.mark.gpu
def test_planted_mismatches_through_tracker_bearings(gpu_ctx):
    """the bearings the tracker hands out (ov2_tracker_last_keypoints) of a keyframe and a current frame with 25 planted mismatches
    go through the chain: every planted mismatch is removed, and nothing is removed that the specification keeps"""
    import ov2slam_amd
    from ov2slam_amd import keyframe, pose, synth
    w, h, K = 376, 240, (300.0, 300.0, 188.0, 120.0)
    rng = np.random.default_rng(33)
    n0 = 140
    Rw = E5._rot(rng, 0.08)
    t = np.array([0.9, 0.1, 0.2])
    t /= np.sqrt((t * t).sum())
    px2 = np.stack([rng.uniform(40, w - 40, n0), rng.uniform(40, h - 40, n0)], axis=1)
    depth = rng.uniform(4.0, 9.0, n0)
    x2 = np.stack([(px2[:, 0] - K[2]) / K[0] * depth, (px2[:, 1] - K[3]) / K[1] * depth, depth], axis=1)
    x1 = x2 @ Rw.T + t
    px1 = np.stack([K[0] * x1[:, 0] / x1[:, 2] + K[2], K[1] * x1[:, 1] / x1[:, 2] + K[3]], axis=1)
    planted = np.zeros(n0, bool)
    planted[rng.choice(n0, 25, replace=False)] = True
    px1[planted, 1] += rng.choice([-1.0, 1.0], 25) * rng.uniform(15, 30, 25)     # t is nearly along x: across the epipolar lines
    inside = (px1[:, 0] > 20) & (px1[:, 0] < w - 20) & (px1[:, 1] > 20) & (px1[:, 1] < h - 20)
    px1, px2, planted = px1[inside], px2[inside], planted[inside]
    n = len(px1)
    px1 = (px1 + rng.normal(0, 0.3, px1.shape)).astype(np.float32)
    px2 = (px2 + rng.normal(0, 0.3, px2.shape)).astype(np.float32)
    img = synth.frame_pair(w, h, seed=3)[0]
    bvs = []
    for px in (px1, px2):
        vt = ov2slam_amd.VisualFrontEndTracker(gpu_ctx, w, h, use_clahe=False, nbmaxkps=256)
        vt.setCalibration(ov2slam_amd.CameraCalibration(gpu_ctx, "pinhole", *K))
        vt.trackFrame(img, np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), None)
        out, st, _ = vt.trackFrame(img, px, px, np.ones(n, np.uint8))       # the same image: a tracked point stays where it is
        _, bv = vt.lastKeypoints(n)
        vt.close()
        bvs.append((np.asarray(bv, np.float64), (st & 1) > 0, out))
    good = bvs[0][1] & bvs[1][1]
    assert good.sum() >= 80
    bv1, bv2, planted = bvs[0][0][good], bvs[1][0][good], planted[good]
    u1, u2 = bvs[0][2][good].astype(np.float32), bvs[1][2][good].astype(np.float32)
    m = int(good.sum())
    ids = (7 * np.arange(m) + 3).astype(int)
    order = rng.permutation(m)                                                  # the frame's map order
    ident = np.array(KF._ID7)
    kf = dict(id=1, time=0.0, Tcw=ident, Twc=ident, nb3dkps=0,
              kps={int(ids[i]): dict(lmid=int(ids[i]), unpx=(u1[i, 0], u1[i, 1]), bv=tuple(bv1[i])) for i in range(m)})
    cur = dict(id=3, time=0.1, Twc=ident, localba_is_on=False, nbkfs=3, seed=5,
               kps={int(ids[i]): dict(lmid=int(ids[i]), px=(u2[i, 0], u2[i, 1]), unpx=(u2[i, 0], u2[i, 1]), bv=tuple(bv2[i]), is3d=False)
                    for i in order})
    P = R.make_P(n_rows=100, K=K, threshold=pose.epipolar_threshold(3.0, K[0], K[1]))
    want = R.spec(P, cur, kf, with_ld=True)
    assert not want["fragile"][np.asarray(want["search"]["consumed_rows"], np.int64)].any()
    got = keyframe.epipolar_filter(gpu_ctx, _params(P), R.flatten(cur, kf))
    assert got["action"] == want["action"] == R.FILTERED and got["m"] == m
    assert np.array_equal(got["removed"], want["removed"])
    lm = np.array([k["lmid"] for k in cur["kps"].values()])
    removed = set(lm[got["removed"] != 0].tolist())
    assert set(ids[planted].tolist()) <= removed
    assert removed <= set(lm[want["removed"] != 0].tolist())
