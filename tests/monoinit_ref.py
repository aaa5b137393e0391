"""numpy specification of the device mono initialisation chain (csrc/monoinit.hip, ov2_mono_init[_batch]) as include/ov2slam_hip.h
states it: trackMono's un-initialised branch (src/visual_front_end.cpp:98-113) with VisualFrontEnd::checkReadyForInit (:855-984),
composed from the pieces that are already specified -- kfreq_ref.replay_parallax (p0, :857), epifilter_ref.join (the join of :893),
fivept_ref.draw_samples / search (the 5-point search) and computepose_ref.pose_from_model (Frame::setTwc) -- plus two restatements
of its own, operation by operation: the rotation-compensated parallax of :908-913 (rot_dist: K as a MATRIX, not
projectCamToImage) and the initial pose of :968-973 (init_pose).  Neither is pinned against an Eigen build.

A scene is (P, cur, kf): P the parameters (dict: fkf = kfreq_ref.make_params(...), max_iterations, threshold, probability, n_rows,
min_2d_kps); cur / kf the dict-based frames of kfreq_ref / epifilter_ref (`kps` in the map's iteration order, the keyframe's
keypoints with a bearing `bv` too) and on cur `seed`.  scenes() are the named scenes, each built to hit one action or one side of
one comparison.

route() is the cycle of separate calls that ov2_btracker_mono_init replaces, on a LockstepTracker whose frames are resident."""
import functools

import numpy as np

from tests import epifilter_ref as EF
from tests import fivept_ref as E5
from tests import kfreq_ref as KF
from tests.computepose_ref import pose_from_model
from tests.tri_ref import D, F32, matvec, pt_dist

RESET, LOW_PARALLAX, TOO_FEW_KPS, TOO_FEW_MATCHES, LOW_ROT_PARALLAX, NO_MODEL, READY = range(7)
ACTIONS = {RESET: "RESET", LOW_PARALLAX: "LOW_PARALLAX", TOO_FEW_KPS: "TOO_FEW_KPS", TOO_FEW_MATCHES: "TOO_FEW_MATCHES",
           LOW_ROT_PARALLAX: "LOW_ROT_PARALLAX", NO_MODEL: "NO_MODEL", READY: "READY"}


# ---- the two restatements ---------------------------------------------------------------------------------------------------------
def k_times(K, v):
    """K * v, K = [fx 0 cx; 0 fy cy; 0 0 1] as Eigen's fixed 3 x 3 by 3 coefficient product: every coefficient the serial sum
    (k0 x + k1 y) + k2 z, the zero entries included"""
    fx, fy, cx, cy = (D(c) for c in K)
    z, o = D(0), D(1)
    x, y, w = v
    return ((fx * x + z * y) + cx * w, (z * x + fy * y) + cy * w, (z * x + z * y) + o * w)


def rot_dist(K, R, bv, kf_unpx):
    """:908-913: cv::norm(Point2f(u.x / u.z, u.y / u.z) - kfkp.unpx_), u = K (Rkfcur bv) -> float64"""
    u = k_times(K, matvec(R, tuple(D(c) for c in bv)))
    rotpx = (F32(u[0] / u[2]), F32(u[1] / u[2]))                               # f32
    return pt_dist(rotpx, kf_unpx)


def rot_parallax(P, cur, kf):
    """:887-923 -> (sum as the reference's float, nbparallax): serial in the map's order, sum = (float)((double)sum + d)"""
    R = KF.rkfcur(kf["Tcw"], cur["Twc"])
    s, nb = F32(0), 0
    with np.errstate(all="ignore"):
        for kp in cur["kps"].values():
            kfkp = kf["kps"].get(kp["lmid"])
            if kfkp is None:
                continue
            s = F32(D(s) + rot_dist(P["fkf"]["K"], R, kp["bv"], kfkp["unpx"]))   # f32, :913
            nb += 1
    return s, nb


def init_pose(model):
    """:968-973 from the unrefined model: [0.25 tkfc / |tkfc|, q(Rkfc)] -> (7,)"""
    m = np.asarray(model, np.float64).reshape(12)
    with np.errstate(all="ignore"):
        nt = np.sqrt((m[9] * m[9] + m[10] * m[10]) + m[11] * m[11])
        t = [(m[9] / nt) * D(0.25), (m[10] / nt) * D(0.25), (m[11] / nt) * D(0.25)]
    return np.array(t + list(pose_from_model(m)[3:7]), np.float64)


# ---- the function -----------------------------------------------------------------------------------------------------------------
def spec(P, cur, kf, with_ld=False):
    """the result of ov2_mono_init, field by field; also `search` (fivept_ref.search's dict, None when the search was not called),
    `samples`, bv1 / bv2, `prep` and, with_ld, `fragile` (fivept_ref.fragile_rows of the table)"""
    kps = list(cur["kps"].values())
    n = len(kps)
    finit = F32(P["fkf"]["finit_parallax"])
    r = dict(action=RESET, nb2dkps=sum(1 for k in kps if not k["is3d"]), p0=F32(0), p0_n=0, p0_n_distinct=0, p0_n_nonfinite=0, m=0,
             p1=F32(0), status=0, best_row=-1, iterations=0, rows_consumed=0, score=D(0), n_inliers=0, n_outliers=0, model=np.zeros(12),
             n_removed=0, pose_refined=0, Twc_init=np.zeros(7), removed=np.zeros(n, np.uint8), pair_cur=np.zeros(0, np.int32),
             search=None, samples=None, bv1=None, bv2=None, prep=None, fragile=None)
    if r["nb2dkps"] < int(P["min_2d_kps"]):                                    # :100
        return r
    pm = KF.replay_parallax(P["fkf"], cur, kf, False, True, False)             # :857
    r.update(action=LOW_PARALLAX, p0=F32(pm["parallax"]), p0_n=pm["n"], p0_n_distinct=pm["n_distinct"], p0_n_nonfinite=pm["n_nonfinite"])
    if not D(r["p0"]) > D(finit):                                              # :861
        return r
    if n < 8:                                                                  # :873
        r["action"] = TOO_FEW_KPS
        return r
    pair_cur, bv1, bv2 = EF.join(cur, kf, False)
    s, m = rot_parallax(P, cur, kf)
    assert m == len(pair_cur)
    r.update(action=TOO_FEW_MATCHES, m=m, pair_cur=pair_cur, bv1=bv1, bv2=bv2)
    if m < 8:                                                                  # :917
        return r
    with np.errstate(all="ignore"):
        r["p1"] = F32(s / F32(m))                                              # :923
    if r["p1"] < finit:                                                        # :925
        r["action"] = LOW_ROT_PARALLAX
        return r
    samples = E5.draw_samples(int(cur["seed"]), m, P["n_rows"])
    prep = E5.prepare(bv1, bv2, samples)
    sr = E5.search(bv1, bv2, samples, P["max_iterations"], P["threshold"], P["probability"], prep=prep)
    r.update(action=NO_MODEL, search=sr, samples=samples, prep=prep, status=sr["status"], best_row=sr["best_row"],
             iterations=sr["iterations"], rows_consumed=sr["rows_consumed"], score=D(sr["score"]), n_inliers=sr["n_inliers"],
             n_outliers=len(sr["outliers"]), model=np.asarray(sr["model"], np.float64))
    if with_ld:
        r["fragile"] = E5.fragile_rows(prep, E5.prepare(bv1, bv2, samples, np.longdouble), P["threshold"])
    if sr["status"] != 0:                                                      # :956
        return r
    r["action"] = READY
    r["removed"][pair_cur[sr["outliers"]]] = 1                                 # :962-965, no 50 % rule
    r["n_removed"] = len(sr["outliers"])
    r["Twc_init"] = init_pose(r["model"])                                      # :968-973
    return r


def flatten(cur, kf):
    """the ov2_mono_init_item of a scene: kfreq_ref.flatten plus kf_bv (in the order of kf_lmid) and seed"""
    item = KF.flatten(cur, kf)
    ids = sorted(kf["kps"])
    item.update(kf_bv=np.array([kf["kps"][i]["bv"] for i in ids], np.float64).reshape(len(ids), 3), seed=int(cur["seed"]))
    return item


# ---- the route of separate calls on a tracker with resident frames -----------------------------------------------------------------
NOT_REQUESTED, NO_KEYFRAME = 7, 8
REC_KEYS = ("action", "nb2dkps", "p0", "p0_n", "p0_n_distinct", "p0_n_nonfinite", "m", "p1", "status", "best_row", "iterations",
            "rows_consumed", "score", "n_inliers", "n_outliers", "model", "n_removed", "pose_refined", "Twc_init")


def zero_record(action):
    return dict(action=action, nb2dkps=0, p0=F32(0), p0_n=0, p0_n_distinct=0, p0_n_nonfinite=0, m=0, p1=F32(0), status=0, best_row=-1,
                iterations=0, rows_consumed=0, score=D(0), n_inliers=0, n_outliers=0, model=np.zeros(12), n_removed=0, pose_refined=0,
                Twc_init=np.zeros(7))


def route(ctx, t, cal, na, do, seeds, P, kf, removed):
    """what LockstepTracker.monoInit does, by the calls that existed before it: per requested item getFrame and
    ov2_compute_keypoints, ov2_parallax_batch for p0, the join and the K rotbv parallax on the host (rot_dist), the table of
    ov2_epipolar_draw_samples, ov2_epipolar_ransac_batch, ov2_pose_from_model, then updateFrame with one REMOVE op per outlier,
    setPose and resetMotion per item.  t: the LockstepTracker; cal: its CameraCalibration; kf[b]: None or dict(lmid ascending, unpx,
    bv, Twc) of item b's resident keyframe; removed: (batch, n_max) uint8 to scatter into.  -> (records, removed)"""
    from ov2slam_amd import keyframe, pose
    recs = [zero_record(NOT_REQUESTED if not do[b] else (NO_KEYFRAME if kf[b] is None or len(kf[b]["lmid"]) == 0 else RESET)) for b in range(na)]
    run = [b for b in range(na) if recs[b]["action"] == RESET]
    finit = F32(P["fkf"]["finit_parallax"])
    items = {}
    for b in run:
        fr = t.getFrame(b, from_device=True)
        n = fr["n"]
        unpx, bv = cal.computeKeypoints(fr["px"][:n])
        items[b] = dict(cur_lmid=fr["lmid"][:n], cur_px=fr["px"][:n], cur_unpx=unpx, cur_bv=bv, cur_is3d=fr["is3d"][:n], cur_Twc=t.getPose(b),
                        kf_lmid=kf[b]["lmid"], kf_unpx=kf[b]["unpx"], kf_bv=kf[b]["bv"], kf_Tcw=keyframe.se3_inverse(kf[b]["Twc"]))
        recs[b]["nb2dkps"] = int((items[b]["cur_is3d"] == 0).sum())
        removed[b, :n] = 0
    live = [b for b in run if recs[b]["nb2dkps"] >= int(P["min_2d_kps"])]                  # :100
    par = keyframe.parallax_batch(ctx, P["fkf"], [items[b] for b in live], unrot=0, filter=keyframe.ALL, stat=keyframe.MEDIAN) if live else []
    search = []
    for b, p in zip(live, par):
        it, r = items[b], recs[b]
        r.update(action=LOW_PARALLAX, p0=F32(p["parallax"]), p0_n=p["n"], p0_n_distinct=p["n_distinct"], p0_n_nonfinite=p["n_nonfinite"])
        if not D(r["p0"]) > D(finit):                                          # :861
            continue
        n = len(it["cur_lmid"])
        if n < 8:                                                              # :873
            r["action"] = TOO_FEW_KPS
            continue
        j = np.searchsorted(it["kf_lmid"], it["cur_lmid"])
        hit = (j < len(it["kf_lmid"])) & (it["kf_lmid"][np.minimum(j, len(it["kf_lmid"]) - 1)] == it["cur_lmid"])
        pair_cur = np.nonzero(hit)[0].astype(np.int32)
        Rm = KF.rkfcur(it["kf_Tcw"], it["cur_Twc"])
        s = F32(0)
        with np.errstate(all="ignore"):
            for i in pair_cur:
                s = F32(D(s) + rot_dist(P["fkf"]["K"], Rm, it["cur_bv"][i], tuple(it["kf_unpx"][j[i]])))
        m = len(pair_cur)
        r.update(action=TOO_FEW_MATCHES, m=m)
        if m < 8:                                                              # :917
            continue
        with np.errstate(all="ignore"):
            r["p1"] = F32(s / F32(m))
        if r["p1"] < finit:                                                    # :925
            r["action"] = LOW_ROT_PARALLAX
            continue
        r["action"] = NO_MODEL
        sm = pose.epipolar_draw_samples(int(seeds[b]), m, P["n_rows"])
        search.append((b, pair_cur, dict(bv1=it["kf_bv"][j[pair_cur]], bv2=it["cur_bv"][pair_cur], samples=sm)))
    found = pose.epipolar_ransac_batch(ctx, pose.epipolar_params(P["max_iterations"], P["threshold"], P["probability"]),
                                       [x[2] for x in search]) if search else []
    ops = [[] for _ in range(na)]
    ready = []
    for (b, pair_cur, _), sr in zip(search, found):
        r = recs[b]
        r.update(status=sr["status"], best_row=sr["best_row"], iterations=sr["iterations"], rows_consumed=sr["rows_consumed"],
                 score=D(sr["score"]), n_inliers=sr["n_inliers"], n_outliers=len(sr["outliers"]), model=np.asarray(sr["model"], np.float64))
        if sr["status"] != 0:                                                  # :956
            continue
        out_cur = pair_cur[sr["outliers"]]
        removed[b, out_cur] = 1
        ops[b] = [(int(items[b]["cur_lmid"][i]), 2, None) for i in out_cur]   # OV2_RES_REMOVE
        q = pose.pose_from_model(r["model"])[3:7]
        m_ = r["model"]
        with np.errstate(all="ignore"):
            nt = np.sqrt((m_[9] * m_[9] + m_[10] * m_[10]) + m_[11] * m_[11])
            tt = [(m_[9] / nt) * D(0.25), (m_[10] / nt) * D(0.25), (m_[11] / nt) * D(0.25)]
        r.update(action=READY, n_removed=len(out_cur), Twc_init=np.array(tt + list(q), np.float64))
        ready.append(b)
    if ready:
        upd = t.updateFrame(na, ops)
        for b in ready:
            assert upd[b]["n_removed"] == len(ops[b]) and upd[b]["n_missing"] == 0
            t.setPose(b, recs[b]["Twc_init"])
    for b in run:
        t.resetMotion(b)
    return recs, removed


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
def make_P(*, n_rows=64, max_iterations=100, min_2d_kps=0, finit_parallax=10., K=KF.EUROC_K, threshold=EF.TH):
    return dict(fkf=KF.make_params(K=K, finit_parallax=finit_parallax), max_iterations=max_iterations, threshold=threshold,
                probability=0.99, n_rows=n_rows, min_2d_kps=min_2d_kps)


def gate_scene(raw, rot):
    """identity poses, K = (1, 1, 0, 0), finit_parallax = 20: keypoint i sits at unpx (raw[i], 0) with the bearing (rot[i], 0, 1)
    against a keyframe keypoint at (0, 0), so its plain parallax is float(raw[i]) and its rotation-compensated one float(rot[i]),
    both exactly: p0 is the median of the distinct raw values, p1 the average of rot (exact where the partial sums are floats)"""
    cur, kf = KF.exact_scene([(float(v), 0., 1.) for v in rot])
    for kp, v in zip(cur["kps"].values(), raw):
        kp["unpx"] = (F32(v), F32(0))
    for k in kf["kps"].values():
        k["bv"] = (0., 0., 1.)
    cur.update(seed=5)
    return cur, kf


def _gate_P():
    P = make_P(n_rows=0)
    P["fkf"] = KF._unit_params()                                               # finit_parallax = 20
    return P


def _scene_table():
    """name -> (P, builder).  The seeds are chosen so that the conditions of tests/test_monoinit_reference.py hold; where a scene of
    epifilter_ref has the same join (every keypoint: stereo off) and the same table, it is that scene's seed."""
    nx = lambda v, up: float(np.nextafter(F32(v), F32(np.inf if up else -np.inf)))
    g = EF.geo_scene
    T = {}
    T["nb2dkps_49"] = (make_P(n_rows=16, min_2d_kps=50), lambda: g(12, 60, n3d=11))
    T["nb2dkps_50"] = (make_P(n_rows=16, min_2d_kps=50), lambda: g(12, 60, n3d=10))
    T["p0_below"] = (_gate_P(), lambda: gate_scene([nx(20., False)] * 8, [40.] * 8))
    T["p0_at"] = (_gate_P(), lambda: gate_scene([20.] * 8, [40.] * 8))
    T["p0_above"] = (_gate_P(), lambda: gate_scene([nx(20., True)] * 8, [40.] * 8))
    T["n_cur_7"] = (make_P(n_rows=16), lambda: g(1, 7))
    T["n_cur_8"] = (make_P(n_rows=16), lambda: g(2, 8))
    T["m_7_of_12"] = (make_P(n_rows=16), lambda: g(3, 12, unknown=5))
    T["m_8_of_12"] = (make_P(n_rows=16), lambda: g(4, 12, unknown=4))
    T["n_kf_0"] = (make_P(n_rows=16), lambda: g(6, 12, unknown=12, extra_kf=0))
    # 160 -+ 2^-10 over eight terms: every partial sum is a float, the average 20 -+ 2^-13 exactly
    T["p1_below"] = (_gate_P(), lambda: gate_scene([100.] * 8, [20.] * 7 + [20. - 2. ** -10]))
    T["p1_at"] = (_gate_P(), lambda: gate_scene([100.] * 8, [20.] * 8))
    T["p1_above"] = (_gate_P(), lambda: gate_scene([100.] * 8, [20.] * 7 + [20. + 2. ** -10]))
    T["rotation_only"] = (make_P(n_rows=16), lambda: g(9, 40, rel_rot=(0.0, 0.08, 0.0), rel_t=(0., 0., 0.)))
    T["inliers_9"] = (make_P(n_rows=48), lambda: g(7, 10, outliers=1))
    T["inliers_10"] = (make_P(n_rows=48), lambda: g(8, 10))
    T["mismatches_30_percent"] = (make_P(n_rows=200), lambda: g(100, 60, outliers=18, noise=0.05, scatter=True))
    T["outliers_over_half"] = (make_P(n_rows=200), lambda: g(208, 60, outliers=31, noise=0.05, scatter=True))
    T["quat_w"] = (make_P(n_rows=32), lambda: g(50, 40))
    for ax in "xyz":
        T["quat_%s" % ax] = (make_P(n_rows=32), lambda ax=ax: g(52 + ord(ax), 40, rel_rot=EF._R170[ax]))
    T["size_63_rows_1"] = (make_P(n_rows=1), lambda: g(164, 63, outliers=6, unknown=3))
    T["size_64_rows_64"] = (make_P(n_rows=64), lambda: g(64, 64, outliers=10, unknown=3))
    T["size_65_rows_65"] = (make_P(n_rows=65), lambda: g(65, 65, n3d=50, outliers=5, unknown=4))
    T["size_308_rows_200"] = (make_P(n_rows=200), lambda: g(308, 308, n3d=200, outliers=60, unknown=20))
    return T


_TABLE = _scene_table()
SCENE_NAMES = tuple(_TABLE)
# where a scene sits exactly on a boundary (exactly representable inputs): exempt from the margin conditions
ON_BOUNDARY = ("p0_below", "p0_at", "p0_above", "p1_below", "p1_at", "p1_above")


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
