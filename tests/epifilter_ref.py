"""numpy specification of the device epipolar2d2dFiltering chain (csrc/epifilter.hip, ov2_epipolar_filter[_batch]) as
include/ov2slam_hip.h states it: VisualFrontEnd::epipolar2d2dFiltering (src/visual_front_end.cpp:440-656) composed from the pieces
that are already specified -- kfreq_ref.replay_parallax_wide (the join and the gate's parallax), fivept_ref.draw_samples / search (the
5-point search) and kfreq_ref.sampson (the pass over the 2-D keypoints) -- plus two restatements of its own, operation by operation:
computeFundamentalMat12 (fundamental) and the mono pose update (mono_pose).  Neither is pinned against an Eigen / Sophus build.

A scene is (P, cur, kf): P the parameters (dict: fkf = kfreq_ref.make_params(...), max_iterations, threshold, probability,
fransac_err, mono, n_rows); cur / kf the dict-based frames of kfreq_ref (`kps` in the map's iteration order), the keyframe's keypoints
with a bearing `bv` too, kf["Twc"], and on cur `nbkfs`, `seed` and optionally `nb3dkps` (absent / -1: counted).  scenes() are the
named scenes, each built to hit one branch or one boundary."""
import functools

import numpy as np

from tests import fivept_ref as E5
from tests import kfreq_ref as KF
from tests.computepose_ref import pose_from_model
from tests.tri_ref import D, F32, pose, rotation_matrix, se3_mul

TOO_FEW_KPS, LOW_PARALLAX, NO_MODEL, DEGENERATE, FILTERED = 0, 1, 2, 3, 4
ACTIONS = {TOO_FEW_KPS: "TOO_FEW_KPS", LOW_PARALLAX: "LOW_PARALLAX", NO_MODEL: "NO_MODEL", DEGENERATE: "DEGENERATE", FILTERED: "FILTERED"}


# ---- the two restatements ---------------------------------------------------------------------------------------------------------
def _mul33(A, B):
    """full 3 x 3 product, each sum of three terms serial"""
    return [[(A[r][0] * B[0][c] + A[r][1] * B[1][c]) + A[r][2] * B[2][c] for c in range(3)] for r in range(3)]


def quat_branch(model):
    """which of Eigen's four matrix-to-quaternion branches the rotation of a model takes: 'w' (trace > 0) or the largest diagonal"""
    m = np.asarray(model, np.float64).reshape(12)
    if (m[0] + m[4]) + m[8] > 0.0:
        return "w"
    i = 0
    if m[4] > m[0]:
        i = 1
    if m[8] > m[4 * i]:
        i = 2
    return "xyz"[i]


def fundamental(K, model):
    """computeFundamentalMat12(identity, SE3(Rkfc, tkfc), K) (src/multi_view_geometry.cpp:824-832): K^-T hat(t) R' K^-1 from left to
    right, R' the rotation matrix of the quaternion of Rkfc, K^-1 in closed form -> (9,) row-major"""
    fx, fy, cx, cy = (D(v) for v in K)
    model = np.asarray(model, np.float64).reshape(12)
    q = pose_from_model(model)[3:7]
    Rq = rotation_matrix(tuple(D(v) for v in q))
    ix, iy, mx, my = D(1) / fx, D(1) / fy, -cx / fx, -cy / fy
    z, o = D(0), D(1)
    iK = [[ix, z, mx], [z, iy, my], [z, z, o]]
    iKt = [[ix, z, z], [z, iy, z], [mx, my, o]]
    tx, ty, tz = D(model[9]), D(model[10]), D(model[11])
    hat = [[z, -tz, ty], [tz, z, -tx], [-ty, tx, z]]
    with np.errstate(all="ignore"):
        return np.array(_mul33(_mul33(_mul33(iKt, hat), Rq), iK), np.float64).reshape(9)


def mono_pose(kf_Twc, kf_Tcw, cur_Twc, model):
    """:594-607 from the unrefined model: kf_Twc * SE3(Rkfc, scale * tkfc / |tkfc|), scale = |(kf_Tcw * cur_Twc).translation()| -> (7,)"""
    model = np.asarray(model, np.float64).reshape(12)
    with np.errstate(all="ignore"):
        t = se3_mul(pose(kf_Tcw), pose(cur_Twc))[0]
        scale = np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
        nt = np.sqrt((model[9] * model[9] + model[10] * model[10]) + model[11] * model[11])
        u = (model[9] / nt, model[10] / nt, model[11] / nt)
        q = tuple(D(v) for v in pose_from_model(model)[3:7])
        T = se3_mul(pose(kf_Twc), ((scale * u[0], scale * u[1], scale * u[2]), q))
    return np.array(list(T[0]) + list(T[1]), np.float64)


# ---- the function -----------------------------------------------------------------------------------------------------------------
def join(cur, kf, epifrom3dkps):
    """:492-512 -> (pair_cur, bv1 (m, 3), bv2 (m, 3)): the current keypoints in the map's order"""
    pc, b1, b2 = [], [], []
    for i, kp in enumerate(cur["kps"].values()):
        if epifrom3dkps and not kp["is3d"]:
            continue
        kfkp = kf["kps"].get(kp["lmid"])
        if kfkp is None:
            continue
        pc.append(i); b1.append(kfkp["bv"]); b2.append(kp["bv"])
    return np.array(pc, np.int32), np.array(b1, np.float64).reshape(-1, 3), np.array(b2, np.float64).reshape(-1, 3)


def spec(P, cur, kf, with_ld=False):
    """the result of ov2_epipolar_filter, field by field; also `search` (fivept_ref.search's dict, None when the search was not
    called), `samples`, bv1 / bv2 and, with_ld, `fragile` (fivept_ref.fragile_rows of the table)"""
    kps = list(cur["kps"].values())
    n = len(kps)
    nb3d = int(cur.get("nb3dkps", -1))
    if nb3d < 0:
        nb3d = sum(1 for k in kps if k["is3d"])
    epifrom3d = bool(P["fkf"]["stereo"]) and nb3d > 30
    do_opt = bool(P["mono"]) and int(cur["nbkfs"]) > 2 and nb3d < 30
    pw = KF.replay_parallax_wide(P["fkf"], cur, kf, epifrom3d)
    pair_cur, bv1, bv2 = join(cur, kf, epifrom3d)
    m = len(pair_cur)
    assert m == pw["n"]
    r = dict(action=NO_MODEL, m=m, epifrom3dkps=int(epifrom3d), do_optimize=int(do_opt), nb3dkps=nb3d, parallax=F32(pw["parallax"]),
             status=0, best_row=-1, iterations=0, rows_consumed=0, score=D(0), n_inliers=0, n_outliers=0, model=np.zeros(12),
             F=np.zeros(9), n_removed_ransac=0, n_removed_sampson=0, removed=np.zeros(n, np.uint8), pair_cur=pair_cur,
             err=np.zeros(n, np.float32), pose_from_model=0, Twc_model=np.zeros(7), search=None, samples=None, bv1=bv1, bv2=bv2,
             fragile=None)
    if n < 8:                                                                  # :462
        r["action"] = TOO_FEW_KPS
        return r
    if D(r["parallax"]) < D(2) * D(F32(P["fransac_err"])):                    # :530
        r["action"] = LOW_PARALLAX
        return r
    samples = E5.draw_samples(int(cur["seed"]), m, P["n_rows"]) if m >= 8 else np.zeros((0, 8), np.int32)
    prep = E5.prepare(bv1, bv2, samples)
    s = E5.search(bv1, bv2, samples, P["max_iterations"], P["threshold"], P["probability"], prep=prep)
    r.update(search=s, samples=samples if m >= 8 else None, status=s["status"], best_row=s["best_row"], iterations=s["iterations"],
             rows_consumed=s["rows_consumed"], score=D(s["score"]), n_inliers=s["n_inliers"], n_outliers=len(s["outliers"]),
             model=np.asarray(s["model"], np.float64))
    r["prep"] = prep
    if with_ld and m >= 8:
        r["fragile"] = E5.fragile_rows(prep, E5.prepare(bv1, bv2, samples, np.longdouble), P["threshold"])
    if s["status"] != 0:                                                       # :574
        return r
    if D(len(s["outliers"])) > D(0.5) * D(m):                                  # :580
        r["action"] = DEGENERATE
        return r
    r["action"] = FILTERED
    r["removed"][pair_cur[s["outliers"]]] = 1                                  # :587-590
    r["n_removed_ransac"] = len(s["outliers"])
    if do_opt:                                                                 # :594
        r["pose_from_model"] = 1
        r["Twc_model"] = mono_pose(kf["Twc"], kf["Tcw"], cur["Twc"], r["model"])
    if epifrom3d:                                                              # :611-648
        r["F"] = fundamental(P["fkf"]["K"], r["model"])
        for i, kp in enumerate(kps):
            if kp["is3d"]:
                continue
            kfkp = kf["kps"].get(kp["lmid"], dict(unpx=(F32(0), F32(0))))
            e = KF.sampson(r["F"], kp["unpx"], kfkp["unpx"])
            r["err"][i] = e
            if e > F32(P["fransac_err"]):
                r["removed"][i] = 2
        r["n_removed_sampson"] = int((r["removed"] == 2).sum())
    return r


def remove_lmids(cur, res):
    """the lmids the reference removes, in its order: the RANSAC outliers ascending in join order, then the 2-D ids in array order"""
    ids = [k["lmid"] for k in cur["kps"].values()]
    out = [ids[i] for i in res["pair_cur"] if res["removed"][i] == 1]
    return out + [ids[i] for i in range(len(ids)) if res["removed"][i] == 2]


def flatten(cur, kf):
    """the ov2_epifilter_item of a scene: kfreq_ref.flatten plus kf_bv (in the order of kf_lmid), kf_Twc, nbkfs, seed"""
    item = KF.flatten(cur, kf)
    ids = sorted(kf["kps"])
    item.update(kf_bv=np.array([kf["kps"][i]["bv"] for i in ids], np.float64).reshape(len(ids), 3),
                kf_Twc=np.array(kf["Twc"], np.float64), nbkfs=int(cur["nbkfs"]), seed=int(cur["seed"]))
    return item


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
TH = E5.threshold_of(3.0, KF.EUROC_K[0], KF.EUROC_K[1])


def make_P(*, stereo=False, mono=False, n_rows=64, max_iterations=100, fransac_err=3.0, K=KF.EUROC_K, threshold=TH):
    return dict(fkf=KF.make_params(K=K, stereo=stereo), max_iterations=max_iterations, threshold=threshold, probability=0.99,
                fransac_err=fransac_err, mono=mono, n_rows=n_rows)


def _aa(axis_angle):
    a = np.asarray(axis_angle, np.float64)
    th = np.linalg.norm(a)
    if th == 0:
        return np.eye(3)
    k = a / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def _q_of(Rm):
    return pose_from_model(np.concatenate([Rm.reshape(9), np.zeros(3)]))[3:7]


def geo_scene(seed, n_cur, *, unknown=0, n3d=0, outliers=0, outliers_2d=0, rel_rot=(0.02, -0.03, 0.01), rel_t=(0.35, 0.05, 0.1),
              noise=0.3, nbkfs=3, nb3dkps_given=False, extra_kf=5, K=KF.EUROC_K, scatter=False):
    """two views of a cloud of points with a known relative pose (x_kf = R x_cur + t): n_cur current keypoints in a shuffled map
    order, the first n3d of a second shuffle are 3-D, `unknown` of them carry ids the keyframe does not hold, `outliers` of the
    joined 3-D-or-all keypoints (and `outliers_2d` of the joined 2-D ones) are displaced by 25 - 60 px across their epipolar line in
    the current image (scatter: put anywhere in the image instead, so that no second model explains several of them).  The keyframe
    holds extra_kf keypoints the frame does not."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = K
    Rrel, trel = _aa(rel_rot), np.asarray(rel_t, np.float64)
    # world = keyframe camera moved by a small pose, so that no pose is the identity
    Rwk, twk = _aa(rng.normal(0, 0.2, 3)), rng.normal(0, 0.5, 3)              # keyframe camera -> world
    Rwc, twc = Rwk @ Rrel, Rwk @ trel + twk                                    # current camera -> world
    kf_Twc = np.concatenate([twk, _q_of(Rwk)])
    kf_Tcw = np.concatenate([-Rwk.T @ twk, _q_of(Rwk.T)])
    cur_Twc = np.concatenate([twc, _q_of(Rwc)])
    n_all = n_cur + extra_kf
    ids = np.sort(rng.choice(5 * n_all + 8, size=n_all, replace=False)).astype(int)
    cur_ids = rng.choice(ids, size=n_cur, replace=False)                      # a shuffled map order
    kf_only = np.setdiff1d(ids, cur_ids)
    order3d = rng.permutation(n_cur)
    is3d = np.zeros(n_cur, bool)
    is3d[order3d[:n3d]] = True
    unk = np.zeros(n_cur, bool)
    unk[rng.permutation(n_cur)[:unknown]] = True
    # points in the current camera, in front of it
    x2 = np.stack([rng.uniform(-1.5, 1.5, n_cur), rng.uniform(-1.0, 1.0, n_cur), rng.uniform(3.0, 8.0, n_cur)], axis=1)
    x1 = x2 @ Rrel.T + trel
    uv2 = x2[:, :2] / x2[:, 2:3] + rng.normal(0, noise / fx, (n_cur, 2))
    Em = np.array([[0, -trel[2], trel[1]], [trel[2], 0, -trel[0]], [-trel[1], trel[0], 0]]) @ Rrel
    joined = ~unk
    pool_a = np.nonzero(joined & (is3d if n3d > 30 else np.ones(n_cur, bool)))[0]
    pool_b = np.nonzero(joined & ~is3d)[0] if n3d > 30 else np.zeros(0, int)
    bad = np.concatenate([rng.choice(pool_a, outliers, replace=False) if outliers else np.zeros(0, int),
                          rng.choice(pool_b, outliers_2d, replace=False) if outliers_2d else np.zeros(0, int)]).astype(int)
    planted = np.zeros(n_cur, bool)
    planted[bad] = True
    if len(bad) and scatter:
        uv2[bad] = np.stack([rng.uniform(-0.7, 0.7, len(bad)), rng.uniform(-0.45, 0.45, len(bad))], axis=1)
    elif len(bad):
        line = (x1[bad] / np.linalg.norm(x1[bad], axis=1)[:, None]) @ Em
        nrm = line[:, :2] / np.linalg.norm(line[:, :2], axis=1)[:, None]
        uv2[bad] += (rng.uniform(25.0, 60.0, len(bad)) / fx * rng.choice([-1.0, 1.0], len(bad)))[:, None] * nrm
    kf = dict(id=40, time=10.0, Tcw=kf_Tcw, Twc=kf_Twc, nb3dkps=n3d, kps={})
    cur = dict(id=43, time=10.15, Twc=cur_Twc, localba_is_on=False, nbkfs=nbkfs, seed=1000 + seed, planted=planted, kps={})

    def kp_of(uvw, lmid, **kw):
        un = (F32(fx * uvw[0] / uvw[2] + cx), F32(fy * uvw[1] / uvw[2] + cy))
        b = np.array([uvw[0], uvw[1], uvw[2]], np.float64)
        return dict(lmid=int(lmid), unpx=un, bv=tuple(b / np.linalg.norm(b)), **kw)
    for i in range(n_cur):
        lmid = int(cur_ids[i])
        cur["kps"][lmid] = kp_of((uv2[i, 0], uv2[i, 1], 1.0), lmid, px=(F32(10), F32(10)), is3d=bool(is3d[i]))
        if not unk[i]:
            uv1 = x1[i, :2] / x1[i, 2] + rng.normal(0, noise / fx, 2)
            kf["kps"][lmid] = kp_of((uv1[0] * x1[i, 2], uv1[1] * x1[i, 2], x1[i, 2]), lmid)
    for lmid in kf_only:
        kf["kps"][int(lmid)] = kp_of((rng.uniform(-0.5, 0.5), rng.uniform(-0.3, 0.3), 1.0), lmid)
    if nb3dkps_given:
        cur["nb3dkps"] = int(is3d.sum())
    return cur, kf


def gate_scene(par, n=8):
    """identity poses, K = (1, 1, 0, 0): n keypoints of parallax float(par) each, so that the average is float(par) exactly (n a
    power of two)"""
    cur, kf = KF.exact_scene([float(par)] * n)
    for k in kf["kps"].values():
        k["bv"] = (0., 0., 1.)
    kf["Twc"] = np.array(KF._ID7)
    cur.update(nbkfs=3, seed=5, planted=np.zeros(n, bool))
    del cur["nb3dkps"]
    return cur, kf


def _gate_P():
    P = make_P(n_rows=0, fransac_err=3.0)
    P["fkf"] = KF._unit_params()
    return P


_R170 = {"x": (np.deg2rad(170.), 0, 0), "y": (0, np.deg2rad(170.), 0), "z": (0, 0, np.deg2rad(170.))}


def _scene_table():
    """name -> (P, builder).  The seeds are chosen so that the conditions of tests/test_epifilter_reference.py hold."""
    nx = lambda v, up: float(np.nextafter(F32(v), F32(np.inf if up else -np.inf)))
    T = {}
    T["n_cur_7"] = (make_P(n_rows=16), lambda: geo_scene(1, 7))
    T["n_cur_8"] = (make_P(n_rows=16), lambda: geo_scene(2, 8))
    T["m_7_of_12"] = (make_P(n_rows=16), lambda: geo_scene(3, 12, unknown=5))
    T["m_8_of_12"] = (make_P(n_rows=16), lambda: geo_scene(4, 12, unknown=4))
    for nb in (30, 31):
        T["stereo_nb3d_%d_given" % nb] = (make_P(stereo=True, n_rows=32), lambda nb=nb: geo_scene(10 + nb, 64, n3d=nb, nb3dkps_given=True))
        T["stereo_nb3d_%d_counted" % nb] = (make_P(stereo=True, n_rows=32), lambda nb=nb: geo_scene(20 + nb, 64, n3d=nb))
    T["gate_below"] = (_gate_P(), lambda: gate_scene(nx(6., False)))
    T["gate_at"] = (_gate_P(), lambda: gate_scene(6.))
    T["gate_above"] = (_gate_P(), lambda: gate_scene(nx(6., True)))
    T["m_0_nan_parallax"] = (make_P(n_rows=16), lambda: geo_scene(5, 12, unknown=12))
    T["n_kf_0"] = (make_P(n_rows=16), lambda: geo_scene(6, 12, unknown=12, extra_kf=0))
    T["inliers_9"] = (make_P(n_rows=48), lambda: geo_scene(7, 10, outliers=1))
    T["inliers_10"] = (make_P(n_rows=48), lambda: geo_scene(8, 10))
    T["outliers_half"] = (make_P(n_rows=200), lambda: geo_scene(100, 60, outliers=30, noise=0.05, scatter=True))
    T["outliers_half_plus_1"] = (make_P(n_rows=200), lambda: geo_scene(208, 60, outliers=31, noise=0.05, scatter=True))
    T["stereo_2d_unknown_to_keyframe"] = (make_P(stereo=True, n_rows=48),
                                          lambda: geo_scene(11, 80, n3d=45, unknown=9, outliers=5, outliers_2d=6))
    for nbkfs in (2, 3):
        for nb in (29, 30):
            T["mono_nbkfs_%d_nb3d_%d" % (nbkfs, nb)] = (make_P(mono=True, n_rows=48),
                                                        lambda nbkfs=nbkfs, nb=nb: geo_scene({(3, 29): 175}.get((nbkfs, nb), 40 + 2 * nbkfs + nb), 60, n3d=nb, nbkfs=nbkfs))
    T["mono_quat_w"] = (make_P(mono=True, n_rows=32), lambda: geo_scene(50, 40))
    T["stereo_quat_w"] = (make_P(stereo=True, n_rows=32), lambda: geo_scene(51, 60, n3d=40, outliers_2d=4))
    for ax in "xyz":
        T["mono_quat_%s" % ax] = (make_P(mono=True, n_rows=32), lambda ax=ax: geo_scene(52 + ord(ax), 40, rel_rot=_R170[ax]))
        T["stereo_quat_%s" % ax] = (make_P(stereo=True, n_rows=32),
                                    lambda ax=ax: geo_scene(56 + ord(ax), 60, n3d=40, outliers_2d=4, rel_rot=_R170[ax]))
    T["size_63_rows_1"] = (make_P(n_rows=1), lambda: geo_scene(164, 63, outliers=6, unknown=3))
    T["size_64_rows_64"] = (make_P(n_rows=64), lambda: geo_scene(64, 64, outliers=10, unknown=3))
    T["size_65_rows_65"] = (make_P(stereo=True, n_rows=65), lambda: geo_scene(65, 65, n3d=50, outliers=5, outliers_2d=3, unknown=4))
    T["size_308_rows_200"] = (make_P(stereo=True, n_rows=200),
                              lambda: geo_scene(308, 308, n3d=200, outliers=60, outliers_2d=30, unknown=20))
    return T


_TABLE = _scene_table()
SCENE_NAMES = tuple(_TABLE)
# where a scene sits exactly on a boundary (exactly representable inputs): exempt from the 1e-9 margin condition
ON_BOUNDARY = ("gate_below", "gate_at", "gate_above")


@functools.lru_cache(maxsize=None)
def scene(name):
    """(P, cur, kf) of a named scene; built once, shared and never changed"""
    P, build = _TABLE[name]
    cur, kf = build()
    return P, cur, kf


@functools.lru_cache(maxsize=None)
def expected(name, with_ld=False):
    P, cur, kf = scene(name)
    return spec(P, cur, kf, with_ld=with_ld)
