"""numpy float64 restatement of the mapper's keyframe triangulation (the reference's src/mapper.cpp:191-461) as
include/ov2slam_hip.h specifies it for ov2_triangulate_keyframe: Mapper::triangulateStereo, then Mapper::triangulateTemporal,
with MultiViewGeometry::triangulate as the OpenGV build runs it (triangulate2, src/multi_view_geometry.cpp:53-100).

Two forms:
  replay()     (a) the two reference loops literally, in loop order, over a minimal dict-based map (keypoints, map points with
               observer sets, keyframes with both poses), applying every map mutation as it happens;
  keyframe()   (b) the per-keypoint form that k_triangulate (ov2slam_amd/csrc/triangulate.hip) implements, one keypoint at a time
               and independent of every other.
tests/test_tri_reference.py checks that both produce the same actions, bit for bit.

Arithmetic: np.float64 scalars (IEEE division by zero, NaN propagation), no fused multiply-add; every narrowing to float32 of the
reference is marked `# f32`.  Sums of three products run serially ((a0 + a1) + a2): the canonical choice of DESIGN.md 2 where
Eigen's order depends on its vectorisation.  Poses are [tx ty tz qx qy qz qw] like the BA structs."""
import numpy as np

D = np.float64
F32 = np.float32

ST_STEREO_TRIED, ST_STEREO_OK, ST_TEMPORAL_TRIED, ST_TEMPORAL_OK, ST_NO_MOTION, ST_REMOVE_OBS = 1, 2, 4, 8, 16, 32


# ---- Sophus / Eigen ------------------------------------------------------------------------------------------------------------
def dot3(a, b):
    return (D(a[0]) * D(b[0]) + D(a[1]) * D(b[1])) + D(a[2]) * D(b[2])


def cross(a, b):
    """Eigen's cross (Eigen/src/Geometry/OrthoMethods.h)"""
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def q_normalize(x, y, z, w):
    """SO3's constructor: normalize() (so3.hpp:297-303, :483-489); squaredNorm in serial order"""
    n = np.sqrt(((x * x + y * y) + z * z) + w * w)
    return (x / n, y / n, z / n, w / n)


def so3_mul(a, b):
    """so3.hpp:329-343, then the SO3 constructor"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    w = aw * bw - ax * bx - ay * by - az * bz
    x = aw * bx + ax * bw + ay * bz - az * by
    y = aw * by + ay * bw + az * bx - ax * bz
    z = aw * bz + az * bw + ax * by - ay * bx
    return q_normalize(x, y, z, w)


def so3_inv(q):
    """so3.hpp:229-231: the conjugate through the SO3 constructor"""
    return q_normalize(-q[0], -q[1], -q[2], q[3])


def so3_act(q, p):
    """so3.hpp:362-371: p + w uv + q x uv, uv = 2 (q x p)"""
    qv = (q[0], q[1], q[2])
    uv = cross(qv, p)
    uv = (uv[0] + uv[0], uv[1] + uv[1], uv[2] + uv[2])
    c = cross(qv, uv)
    return tuple((p[i] + q[3] * uv[i]) + c[i] for i in range(3))


def pose(T):
    """[tx ty tz qx qy qz qw] as held (no renormalisation) -> (t, q)"""
    T = [D(v) for v in T]
    return (tuple(T[0:3]), tuple(T[3:7]))


def se3_mul(A, B):
    """se3.hpp:308-312"""
    ta, qa = A
    tb, qb = B
    r = so3_act(qa, tb)
    return (tuple(ta[i] + r[i] for i in range(3)), so3_mul(qa, qb))


def se3_inv(A):
    """se3.hpp:208-211"""
    t, q = A
    qi = so3_inv(q)
    return (so3_act(qi, (t[0] * D(-1), t[1] * D(-1), t[2] * D(-1))), qi)


def se3_act(A, p):
    """se3.hpp:325-328"""
    t, q = A
    r = so3_act(q, p)
    return (r[0] + t[0], r[1] + t[1], r[2] + t[2])


def rotation_matrix(q):
    """Eigen's QuaternionBase::toRotationMatrix, no renormalisation (so3.hpp matrix())"""
    x, y, z, w = q
    tx, ty, tz = D(2) * x, D(2) * y, D(2) * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return ((D(1) - (tyy + tzz), txy - twz, txz + twy),
            (txy + twz, D(1) - (txx + tzz), tyz - twx),
            (txz - twy, tyz + twx, D(1) - (txx + tyy)))


def matvec(M, v):
    return tuple((M[i][0] * v[0] + M[i][1] * v[1]) + M[i][2] * v[2] for i in range(3))


def norm3(v):
    return np.sqrt(dot3(v, v))


# ---- OpenGV triangulate2 ---------------------------------------------------------------------------------------------------------
def triangulate2(R12, t12, f1, f2):
    """opengv::triangulation::triangulate2 (the public OpenGV source), as MultiViewGeometry::opengvTriangulate2 calls it
    (src/multi_view_geometry.cpp:85-100): R12 / t12 are the Tlr handed to triangulate"""
    f1 = tuple(D(v) for v in f1)
    f2u = matvec(R12, tuple(D(v) for v in f2))
    b0, b1 = dot3(t12, f1), dot3(t12, f2u)
    a00, a10 = dot3(f1, f1), dot3(f1, f2u)
    a01, a11 = -a10, -dot3(f2u, f2u)
    invdet = D(1) / (a00 * a11 - a10 * a01)            # Eigen compute_inverse<.., 2>: 1 / determinant()
    i00, i10, i01, i11 = a11 * invdet, -a10 * invdet, -a01 * invdet, a00 * invdet
    l0 = i00 * b0 + i01 * b1
    l1 = i10 * b0 + i11 * b1
    xm = (l0 * f1[0], l0 * f1[1], l0 * f1[2])
    xn = tuple(t12[i] + l1 * f2u[i] for i in range(3))
    return tuple((xm[i] + xn[i]) / D(2) for i in range(3))


# ---- cv::Point2f projections and distances ----------------------------------------------------------------------------------------
def project(K, p):
    """CameraCalibration::projectCamToImage (src/camera_calibration.cpp:243-252): double math, cv::Point2f result"""
    fx, fy, cx, cy = (D(v) for v in K)
    invz = D(1) / p[2]
    x, y = p[0] * invz, p[1] * invz
    return (F32(fx * x + cx), F32(fy * y + cy))                 # f32


def pt_dist(a, b):
    """cv::norm(a - b) of two cv::Point2f: the difference in float, the norm in double"""
    dx, dy = F32(F32(a[0]) - F32(b[0])), F32(F32(a[1]) - F32(b[1]))    # f32
    return np.sqrt(D(dx) * D(dx) + D(dy) * D(dy))


# ---- per-keypoint form (b) --------------------------------------------------------------------------------------------------------
def stereo_point(P, Twc, unpx, bv, runpx, rbv):
    """Mapper::triangulateStereo's loop body (src/mapper.cpp:405-456) -> (ok, wpt, invdepth)"""
    Tlr = pose(P["Tlr"])
    Tcic0 = pose(P["Tcic0"])
    Trl = se3_inv(Tlr)                                           # :379
    if P["rect"]:
        disp = F32(F32(unpx[0]) - F32(runpx[0]))                 # f32  :411
        if disp < 0.:
            return False, None, None
        z = F32(D(P["K"][0]) * norm3(Tcic0[0]) / D(np.abs(disp)))   # f32  :417
        iK = [D(v) for v in P["iK"]]
        v = (D(F32(unpx[0])), D(F32(unpx[1])), D(1))
        left = tuple((D(z) * iK[3 * i] * v[0] + D(z) * iK[3 * i + 1] * v[1]) + D(z) * iK[3 * i + 2] * v[2] for i in range(3))
    else:
        left = triangulate2(rotation_matrix(Tlr[1]), Tlr[0], bv, rbv)
    right = se3_act(Trl, left)
    if left[2] < 0.1 or right[2] < 0.1:
        return False, None, None
    ldist = F32(pt_dist(project(P["K"], left), unpx))            # f32
    rdist = F32(pt_dist(project(P["Kr"], se3_act(Tcic0, left)), runpx))   # f32
    emax = F32(P["fmax_reproj_err"])
    if ldist > emax or rdist > emax:
        return False, None, None
    return True, se3_act(pose(Twc), left), D(1) / left[2]


def temporal_point(P, Twcj, unpx, bv, src_Twc, src_Tcw, kfunpx, kfbv):
    """Mapper::triangulateTemporal's loop body from the relative pose on (src/mapper.cpp:273-333) -> (status bits, wpt, invdepth)"""
    Tcicj = se3_mul(pose(src_Tcw), pose(Twcj))                   # :278
    Tcjci = se3_inv(Tcicj)                                       # :280
    R = rotation_matrix(Tcicj[1])                                # :281
    if P["stereo"] and norm3(Tcicj[0]) < 0.01:                   # :287
        return ST_NO_MOTION, None, None
    parallax = pt_dist(kfunpx, project(P["K"], matvec(R, tuple(D(v) for v in bv))))   # :299-300
    st = ST_TEMPORAL_TRIED
    left = triangulate2(R, Tcicj[0], kfbv, bv)
    right = se3_act(Tcjci, left)
    ok = not (left[2] < 0.1 or right[2] < 0.1)
    if ok:
        ldist = F32(pt_dist(project(P["K"], left), kfunpx))      # f32
        rdist = F32(pt_dist(project(P["K"], right), unpx))       # f32
        emax = F32(P["fmax_reproj_err"])
        ok = not (ldist > emax or rdist > emax)
    if not ok:
        return st | (ST_REMOVE_OBS if parallax > 20. else 0), None, None
    return st | ST_TEMPORAL_OK, se3_act(pose(src_Twc), left), D(1) / left[2]


def keyframe(P, kf):
    """(b): what ov2_triangulate_keyframe returns for one keyframe.  kf: dict of arrays as ov2_tri_keyframe holds them
    (Twc, unpx (n,2) f32, bv (n,3), is_stereo (n,), runpx, rbv, src (n,) int, src_unpx, src_bv, src_Twc (m,7), src_Tcw (m,7)).
    Returns (status (n,) uint8, wpt (n,3) float64, invdepth (n,) float64); points without a result hold zeros."""
    n = len(kf["unpx"])
    status = np.zeros(n, np.uint8)
    wpt = np.zeros((n, 3), np.float64)
    inv = np.zeros(n, np.float64)
    with np.errstate(all="ignore"):
        for i in range(n):
            st = 0
            if kf["is_stereo"][i]:
                st = ST_STEREO_TRIED
                ok, w, d = stereo_point(P, kf["Twc"], kf["unpx"][i], kf["bv"][i], kf["runpx"][i], kf["rbv"][i])
                if ok:
                    st |= ST_STEREO_OK
                    wpt[i], inv[i] = w, d
            s = int(kf["src"][i])
            if not (st & ST_STEREO_OK) and s >= 0:
                t, w, d = temporal_point(P, kf["Twc"], kf["unpx"][i], kf["bv"][i], kf["src_Twc"][s], kf["src_Tcw"][s],
                                         kf["src_unpx"][i], kf["src_bv"][i])
                st |= t
                if t & ST_TEMPORAL_OK:
                    wpt[i], inv[i] = w, d
            status[i] = st
    return status, wpt, inv


def actions_from_status(kfid, lmids, status, wpt, inv, src_kfids=None):
    """the map mutations a caller replays from the per-keypoint results, in the reference's loop order: the stereo loop over the
    stereo keypoints, then the temporal loop over the keypoints still 2-D"""
    acts = []
    for i, st in enumerate(status):
        if st & ST_STEREO_TRIED:
            acts.append(("update", int(lmids[i]), _bits(wpt[i]), _bits([inv[i]])) if st & ST_STEREO_OK else ("rm_stereo", int(lmids[i])))
    for i, st in enumerate(status):
        if st & ST_TEMPORAL_OK:
            acts.append(("update", int(lmids[i]), _bits(wpt[i]), _bits([inv[i]])))
        elif st & ST_REMOVE_OBS:
            acts.append(("rm_obs", int(lmids[i]), int(kfid)))
    return acts


def _bits(v):
    return tuple(int(x) for x in np.asarray(v, np.float64).view(np.uint64))


# ---- literal replay (a) -----------------------------------------------------------------------------------------------------------
def replay(P, M):
    """(a): Mapper::triangulateStereo then Mapper::triangulateTemporal, loop by loop, on a dict-based map M:
        M["frame"]     {"kfid", "Twc", "Tcw", "kps": [{"lmid", "unpx", "bv", "is3d", "is_stereo", "runpx", "rbv"}]}
        M["kfs"]       {kfid: {"Twc", "Tcw", "kps": {lmid: {"unpx", "bv"}}}}   (the new keyframe included, its kps unused)
        M["mps"]       {lmid: {"is3d", "obs": set of kfids}}
    Mutates M and returns the action list (same format as actions_from_status)."""
    fr, kfs, mps = M["frame"], M["kfs"], M["mps"]
    acts = []

    def kp_of(lmid):
        for kp in fr["kps"]:
            if kp["lmid"] == lmid:
                return kp
        return None

    def update_map_point(lmid, w, d):
        mps[lmid]["is3d"] = True
        kp = kp_of(lmid)
        if kp is not None:
            kp["is3d"] = True
        acts.append(("update", lmid, _bits(w), _bits([d])))

    with np.errstate(all="ignore"):
        # triangulateStereo (:346-461)
        vkps = [dict(kp) for kp in fr["kps"] if kp["is_stereo"]]
        for kp in [k for k in vkps if not k["is3d"] and k["is_stereo"]]:
            ok, w, d = stereo_point(P, fr["Twc"], kp["unpx"], kp["bv"], kp["runpx"], kp["rbv"])
            if not ok:
                kp_of(kp["lmid"])["is_stereo"] = False          # removeStereoKeypointById
                acts.append(("rm_stereo", kp["lmid"]))
                continue
            update_map_point(kp["lmid"], w, d)
        # triangulateTemporal (:191-344)
        vkps = [dict(kp) for kp in fr["kps"] if not kp["is3d"]]
        relkfid = -1
        Tcicj = Tcjci = R = None
        for kp in vkps:
            plm = mps.get(kp["lmid"])
            if plm is None or plm["is3d"]:
                continue
            co = sorted(plm["obs"])
            if len(co) < 2:
                continue
            kfid = co[0]
            if kfid == fr["kfid"] or kfid not in kfs:
                continue
            pkf = kfs[kfid]
            if relkfid != kfid:
                Tcicj = se3_mul(pose(pkf["Tcw"]), pose(fr["Twc"]))
                Tcjci = se3_inv(Tcicj)
                R = rotation_matrix(Tcicj[1])
                relkfid = kfid
            if P["stereo"] and norm3(Tcicj[0]) < 0.01:
                continue
            kfkp = pkf["kps"].get(kp["lmid"])
            if kfkp is None:
                continue
            parallax = pt_dist(kfkp["unpx"], project(P["K"], matvec(R, tuple(D(v) for v in kp["bv"]))))
            left = triangulate2(R, Tcicj[0], kfkp["bv"], kp["bv"])
            right = se3_act(Tcjci, left)
            bad = left[2] < 0.1 or right[2] < 0.1
            if not bad:
                ldist = F32(pt_dist(project(P["K"], left), kfkp["unpx"]))
                rdist = F32(pt_dist(project(P["K"], right), kp["unpx"]))
                bad = ldist > F32(P["fmax_reproj_err"]) or rdist > F32(P["fmax_reproj_err"])
            if bad:
                if parallax > 20.:
                    plm["obs"].discard(fr["kfid"])              # removeMapPointObs
                    fr["kps"] = [k for k in fr["kps"] if k["lmid"] != kp["lmid"]]
                    acts.append(("rm_obs", kp["lmid"], fr["kfid"]))
                continue
            update_map_point(kp["lmid"], se3_act(pose(pkf["Twc"]), left), D(1) / left[2])
    return acts


def inputs_from_map(M):
    """the host's side of the split (src/mapper.cpp:243-295, decided before the stereo pass, which changes none of it): per
    keypoint of the new keyframe its stereo flag, temporal source keyframe (index into a table of the distinct first observers)
    and the source keypoint.  Returns (kf dict for keyframe(), lmids, table kfids)."""
    fr, kfs, mps = M["frame"], M["kfs"], M["mps"]
    n = len(fr["kps"])
    table = []
    src = np.full(n, -1, np.int32)
    su = np.zeros((n, 2), np.float32)
    sb = np.zeros((n, 3), np.float64)
    for i, kp in enumerate(fr["kps"]):
        plm = mps.get(kp["lmid"])
        if kp["is3d"] or plm is None or plm["is3d"] or len(plm["obs"]) < 2:
            continue
        kfid = min(plm["obs"])
        if kfid == fr["kfid"] or kfid not in kfs or kp["lmid"] not in kfs[kfid]["kps"]:
            continue
        if kfid not in table:
            table.append(kfid)
        src[i] = table.index(kfid)
        su[i] = kfs[kfid]["kps"][kp["lmid"]]["unpx"]
        sb[i] = kfs[kfid]["kps"][kp["lmid"]]["bv"]
    kf = dict(Twc=np.asarray(fr["Twc"], np.float64),
              unpx=np.array([kp["unpx"] for kp in fr["kps"]], np.float32).reshape(n, 2),
              bv=np.array([kp["bv"] for kp in fr["kps"]], np.float64).reshape(n, 3),
              is_stereo=np.array([kp["is_stereo"] and not kp["is3d"] for kp in fr["kps"]], np.uint8),
              runpx=np.array([kp["runpx"] for kp in fr["kps"]], np.float32).reshape(n, 2),
              rbv=np.array([kp["rbv"] for kp in fr["kps"]], np.float64).reshape(n, 3),
              src=src, src_unpx=su, src_bv=sb,
              src_Twc=np.array([kfs[k]["Twc"] for k in table], np.float64).reshape(-1, 7),
              src_Tcw=np.array([kfs[k]["Tcw"] for k in table], np.float64).reshape(-1, 7))
    return kf, [kp["lmid"] for kp in fr["kps"]], table


# ---- synthetic scenes --------------------------------------------------------------------------------------------------------------
EUROC = dict(K=(458.654, 457.296, 367.215, 248.375), Kr=(457.587, 456.134, 379.999, 255.238))
KITTI = dict(K=(718.856, 718.856, 607.1928, 185.2157), Kr=(718.856, 718.856, 607.1928, 185.2157))


def _quat(rng, s):
    q = np.concatenate([rng.normal(0, s, 3), [1.0]])
    return q / np.linalg.norm(q)


def _pose(t, q):
    return np.concatenate([np.asarray(t, np.float64), np.asarray(q, np.float64)])


def _inv7(T):
    t, q = se3_inv(pose(T))
    return np.array(list(t) + list(q), np.float64)


def _iK(K):
    fx, fy, cx, cy = K
    return np.linalg.inv(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)).reshape(9)


def make_params(cam=EUROC, *, stereo=True, rect=False, rot=0.02, baseline=0.11, fmax_reproj_err=3.0, seed=0):
    """ov2_tri_params as a dict.  rect: a KITTI-like rectified pair (identity rotation, right K = left K); otherwise a EuRoC-like
    pair whose extrinsic is rotated by ~rot rad.  Tcic0 is Tc0ci.inverse(), like CameraCalibration::setupExtrinsic (:195-198)."""
    rng = np.random.default_rng(seed)
    q = np.array([0, 0, 0, 1.0]) if rect else _quat(rng, rot)
    Tlr = _pose([baseline, 0.0 if rect else rng.normal(0, 0.002), 0.0 if rect else rng.normal(0, 0.002)], q)
    K = cam["K"]
    return dict(stereo=bool(stereo), rect=bool(rect), fmax_reproj_err=float(fmax_reproj_err), K=tuple(K), iK=_iK(K),
                Kr=tuple(K if rect else cam["Kr"]), Tlr=Tlr, Tcic0=_inv7(Tlr))


def _cam_obs(K, iK, pc):
    """(unpx f32, bv) of a camera-frame point: the pixel narrowed like cv::Point2f, the bearing from the exact direction"""
    pc = np.asarray(pc, np.float64)
    u = np.array(project(K, tuple(D(v) for v in pc)), np.float32)
    return u, pc / np.linalg.norm(pc)


def make_map(P, rng, n=300, n_src=4, *, kfid=None, noise=0.0, behind=0.0, p_stereo=0.7, p_src=0.8, motion=0.4,
             no_motion_kf=False, kps_3d=0.0, lone=0.0, missing_src_kp=0.0):
    """a dict-based map for replay() around a new keyframe with n keypoints, n_src earlier keyframes.
    noise: fraction of keypoints whose right or source observation is displaced by 2-40 px (reprojection failures on both sides of
    the parallax threshold); behind: fraction of points placed behind the new camera; no_motion_kf: source keyframe 0 sits at the
    new keyframe's pose (stereo-mode skip); kps_3d / lone / missing_src_kp: host-side ineligibility of the temporal pass."""
    K, Kr, iK = P["K"], P["Kr"], P["iK"]
    kfid = n_src if kfid is None else kfid
    Tcic0 = pose(P["Tcic0"])
    Twc = _pose(rng.normal(0, 1.0, 3), _quat(rng, 0.3))
    Tcw = _inv7(Twc)
    kfs = {}
    for k in range(n_src):
        if no_motion_kf and k == 0:
            T = Twc.copy()
        else:
            dt = rng.normal(0, motion, 3)
            t, _ = se3_act(pose(Twc), tuple(D(v) for v in dt)), None
            T = _pose(t, so3_mul(tuple(Twc[3:]), tuple(_quat(rng, 0.05))))
        kfs[k] = dict(Twc=T, Tcw=_inv7(T), kps={})
    kfs[kfid] = dict(Twc=Twc, Tcw=Tcw, kps={})
    kps, mps = [], {}
    w, h = 2 * K[2], 2 * K[3]
    for i in range(n):
        lmid = 1000 + i
        z = rng.uniform(1.0, 30.0) * (-1 if rng.uniform() < behind else 1)
        u, v = rng.uniform(0, w), rng.uniform(0, h)
        pc = np.array([(u - K[2]) / K[0] * abs(z), (v - K[3]) / K[1] * abs(z), z])
        wp = np.array(se3_act(pose(Twc), tuple(D(x) for x in pc)), np.float64)
        unpx, bv = _cam_obs(K, iK, pc)
        pr = np.array(se3_act(Tcic0, tuple(D(x) for x in pc)))
        runpx, rbv = _cam_obs(Kr, None, pr)
        if P["rect"]:
            runpx[1] = unpx[1]                                   # map_manager.cpp:578
        if rng.uniform() < noise / 2:
            runpx = (runpx + rng.uniform(-40, 40, 2)).astype(np.float32)
            rbv = (rbv + rng.normal(0, 0.02, 3)); rbv /= np.linalg.norm(rbv)
        kp = dict(lmid=lmid, unpx=unpx, bv=bv, is3d=bool(rng.uniform() < kps_3d), is_stereo=bool(P["stereo"] and rng.uniform() < p_stereo),
                  runpx=runpx, rbv=rbv)
        kps.append(kp)
        obs = {kfid}
        if rng.uniform() < p_src and n_src > 0 and rng.uniform() >= lone:
            s = int(rng.integers(0, n_src))
            obs |= {s} | set(int(x) for x in rng.integers(s, n_src, 2))
            if rng.uniform() >= missing_src_kp:
                ps = np.array(se3_act(pose(kfs[s]["Tcw"]), tuple(D(x) for x in wp)))
                su, sb = _cam_obs(K, iK, ps)
                if rng.uniform() < noise / 2:
                    su = (su + rng.uniform(-40, 40, 2)).astype(np.float32)
                    sb = sb + rng.normal(0, 0.02, 3); sb /= np.linalg.norm(sb)
                kfs[s]["kps"][lmid] = dict(unpx=su, bv=sb)
        mps[lmid] = dict(is3d=kp["is3d"], obs=obs, wpt=wp)
    return dict(frame=dict(kfid=kfid, Twc=Twc, Tcw=Tcw, kps=kps), kfs=kfs, mps=mps)


def one_point_kf(P, Twc, pc, *, stereo=False, runpx=None, src=None, src_unpx=None):
    """a keyframe with the single camera-frame point pc: exact observations, optionally overridden; src = (Twc, Tcw) of a source
    keyframe whose observation of the same world point is attached"""
    K, iK = P["K"], P["iK"]
    unpx, bv = _cam_obs(K, iK, pc)
    pr = np.array(se3_act(pose(P["Tcic0"]), tuple(D(x) for x in pc)))
    ru, rbv = _cam_obs(P["Kr"], None, pr)
    if P["rect"]:
        ru[1] = unpx[1]
    if runpx is not None:
        ru = np.asarray(runpx, np.float32)
    kf = dict(Twc=np.asarray(Twc, np.float64), unpx=unpx[None], bv=bv[None], is_stereo=np.array([int(stereo)], np.uint8),
              runpx=ru[None], rbv=rbv[None], src=np.array([-1], np.int32), src_unpx=np.zeros((1, 2), np.float32),
              src_bv=np.zeros((1, 3)), src_Twc=np.zeros((0, 7)), src_Tcw=np.zeros((0, 7)))
    if src is not None:
        sTwc, sTcw = src
        wp = se3_act(pose(Twc), tuple(D(x) for x in pc))
        su, sb = _cam_obs(K, iK, np.array(se3_act(pose(sTcw), wp)))
        if src_unpx is not None:
            su = np.asarray(src_unpx, np.float32)
        kf.update(src=np.array([0], np.int32), src_unpx=su[None], src_bv=sb[None], src_Twc=np.asarray(sTwc, np.float64)[None],
                  src_Tcw=np.asarray(sTcw, np.float64)[None])
    return kf


def crafted_cases():
    """(name, params, keyframe, expected status of its one point) -- one per branch of both passes"""
    out = []
    I = _pose([0, 0, 0], [0, 0, 0, 1])
    Twc = _pose([0.3, -0.2, 0.1], _quat(np.random.default_rng(5), 0.2))
    Pr = make_params(KITTI, rect=True)
    Pu = make_params(EUROC, rect=False, seed=3)
    Pm = make_params(EUROC, stereo=False, seed=3)
    pc = np.array([0.4, -0.3, 6.0])
    u = project(Pr["K"], tuple(pc))
    out.append(("rect_negative_disparity", Pr, one_point_kf(Pr, Twc, pc, stereo=True, runpx=[u[0] + 0.5, u[1]]), ST_STEREO_TRIED))
    out.append(("rect_zero_disparity_nan", Pr, one_point_kf(Pr, Twc, pc, stereo=True, runpx=[u[0], u[1]]), ST_STEREO_TRIED | ST_STEREO_OK))
    out.append(("rect_ok", Pr, one_point_kf(Pr, Twc, pc, stereo=True), ST_STEREO_TRIED | ST_STEREO_OK))
    out.append(("unrect_ok", Pu, one_point_kf(Pu, Twc, pc, stereo=True), ST_STEREO_TRIED | ST_STEREO_OK))
    out.append(("behind_left", Pu, one_point_kf(Pu, Twc, np.array([0.4, -0.3, -6.0]), stereo=True), ST_STEREO_TRIED))
    Pf = make_params(EUROC, rect=False, seed=3)
    Pf["Tlr"] = _pose([0.11, 0.0, 0.05], [0, 0, 0, 1]); Pf["Tcic0"] = _inv7(Pf["Tlr"])
    out.append(("behind_right", Pf, one_point_kf(Pf, Twc, np.array([0.01, 0.0, 0.12]), stereo=True), ST_STEREO_TRIED))
    out.append(("stereo_reproj", Pu, one_point_kf(Pu, Twc, pc, stereo=True,
                                                 runpx=np.array(project(Pu["Kr"], se3_act(pose(Pu["Tcic0"]), tuple(pc)))) + [0, 4.0]),
                ST_STEREO_TRIED))
    # temporal: a source keyframe 0.25 m to the side; the source pixel is moved along the parallax direction so that the
    # rotation-compensated parallax is 19.99 or 20.01 px while the source-side reprojection error stays above the gate
    sT = _pose(se3_act(pose(Twc), (D(-0.13), D(0.01), D(0.0))), so3_mul(tuple(Twc[3:]), tuple(_quat(np.random.default_rng(6), 0.03))))
    src = (sT, _inv7(sT))
    base = one_point_kf(Pm, Twc, pc, src=src)
    Tcicj = se3_mul(pose(src[1]), pose(Twc))
    rot = np.array(project(Pm["K"], matvec(rotation_matrix(Tcicj[1]), tuple(base["bv"][0]))), np.float64)
    d = base["src_unpx"][0].astype(np.float64) - rot
    assert 5 < np.linalg.norm(d) < 15, np.linalg.norm(d)
    for name, par, rm in (("temporal_reproj_parallax_below_20", 19.99, 0), ("temporal_reproj_parallax_above_20", 20.01, ST_REMOVE_OBS)):
        su = (rot + d / np.linalg.norm(d) * par).astype(np.float32)
        out.append((name, Pm, one_point_kf(Pm, Twc, pc, src=src, src_unpx=su), ST_TEMPORAL_TRIED | rm))
    out.append(("temporal_ok", Pm, base, ST_TEMPORAL_TRIED | ST_TEMPORAL_OK))
    out.append(("temporal_behind", Pm, one_point_kf(Pm, Twc, np.array([0.4, -0.3, -6.0]), src=src), ST_TEMPORAL_TRIED))
    same = (Twc.copy(), _inv7(Twc))
    out.append(("no_motion_stereo_mode", Pu, one_point_kf(Pu, Twc, pc, src=same), ST_NO_MOTION))
    # mono mode has no skip: t12 = 0 and f1 == f2u make A singular, the point is NaN and every gate lets it through
    out.append(("no_motion_mono_mode_nan", Pm, one_point_kf(Pm, Twc, pc, src=same), ST_TEMPORAL_TRIED | ST_TEMPORAL_OK))
    bad_r = np.array(project(Pu["Kr"], se3_act(pose(Pu["Tcic0"]), tuple(pc)))) + [0, 6.0]
    out.append(("stereo_rejected_then_temporal_ok", Pu, one_point_kf(Pu, Twc, pc, stereo=True, runpx=bad_r, src=src),
                ST_STEREO_TRIED | ST_TEMPORAL_TRIED | ST_TEMPORAL_OK))
    return out
