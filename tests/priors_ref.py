"""numpy restatement of the places where the reference derives the priors of its KLT calls, as include/ov2slam_hip.h specifies
them for ov2_klt_priors / ov2_stereo_priors: VisualFrontEnd::kltTracking (src/visual_front_end.cpp:156-184) and
MapManager::stereoMatching (src/map_manager.cpp:396-489) with Frame::getSurroundingKeypoints(const Keypoint&)
(src/frame.cpp:594-622).  The projection is tests/match_ref.py's project_dist / in_image; it is not restated here.

Two forms:
  replay_*()   (a) the reference loops literally, over a dict-based frame (`mapkps_`: a dict lmid -> keypoint in the map's
               iteration order, `vgridkps_`: per cell the lmids in insertion order) and a dict-based map (lmid -> world point; a
               missing id is getMapPoint() == nullptr);
  flat_*()     (b) the per-keypoint form that k_prior_frame / k_prior_stereo (ov2slam_amd/csrc/priors.hip) implement on flat arrays:
               a state byte per keypoint (0 = 2-D, 1 = 3-D with a live map point, 2 = 3-D whose map point is gone) and the cell
               tables of ov2_match_keyframe.
tests/test_priors_reference.py checks that both produce the same results, bit for bit.

Arithmetic: np.float64 / np.float32 scalars, no fused multiply-add; the Sophus / Eigen / cv::norm conventions are those of
tests/tri_ref.py.  Poses are [tx ty tz qx qy qz qw] as held; Tcw is the predicted pose, already inverted.

Where the reference is undefined both forms do what the header says: a cell of the 2 x 2 block beyond the grid's last row
(vgridkps_.at() would throw) is skipped.  A keypoint right of the grid's last column would make the reference wrap into the next
row; the flat form skips such a column, and the generators keep every px inside the image, where the two cannot differ.  The frame
form's map_plms_.at(lmid) throws for a 3-D keypoint without a map point: replay_klt raises KeyError, the flat form has no such
state."""
import numpy as np

from tests.match_ref import EUROC, FISHEYE4, RADTAN4, _inv_act, _rand_pose, grid_width, in_image, project_dist
from tests.tri_ref import D, F32, pose, pt_dist, se3_act

RADTAN8 = RADTAN4 + (-0.0091, 0.012, -0.004, 0.0007)
CRAFT_CAM = dict(K=(512.0, 512.0, 384.0, 256.0), img_w=768, img_h=512, ncellsize=32)
I7 = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
BASELINE = (-0.11, 0.0005, -0.0002, 0.001, -0.002, 0.0015, 1.0)      # a plausible Tcic0: 11 cm to the right, a small rotation


def make_params(D=None, model="pinhole", cam=EUROC, klt_use_prior=True, rect=False, Tcic0=BASELINE):
    q = np.asarray(Tcic0[3:], np.float64)
    T = tuple(float(v) for v in Tcic0[:3]) + tuple(float(v) for v in q / np.linalg.norm(q))
    return dict(model=model, K=tuple(cam["K"]), D=None if D is None else tuple(D), img_w=cam["img_w"], img_h=cam["img_h"],
                ncellsize=cam["ncellsize"], klt_use_prior=bool(klt_use_prior), rect=bool(rect), Tcic0=T)


def _w(v):
    return tuple(D(x) for x in v)


def _margin(ev, P, px):
    """smallest distance of a tested projection from an image edge met so far (the fisheye scenes are checked on it)"""
    if ev is not None:
        for v in (px[0], px[1], D(px[0]) - D(P["img_w"]), D(px[1]) - D(P["img_h"])):
            v = abs(float(v))
            if v == v:
                ev["margin"] = min(ev.get("margin", np.inf), v)


# ---- (a) the reference loops ------------------------------------------------------------------------------------------------------
def replay_klt(P, frame, mps):
    """VisualFrontEnd::kltTracking, :156-184 -> {lmid: (prior, has_prior)} in mapkps_ order"""
    out = {}
    T = pose(frame["Tcw"])
    for lmid, kp in frame["mapkps_"].items():
        if P["klt_use_prior"]:
            if kp["is3d"]:
                projpx = project_dist(P, se3_act(T, _w(mps[kp["lmid"]])))       # map_plms_.at(): KeyError when absent
                if in_image(P, projpx):
                    out[lmid] = (projpx, 1)
                    continue
        out[lmid] = (kp["px"], 0)
    return out


def _surrounding(P, frame, kp):
    """Frame::getSurroundingKeypoints(const Keypoint&), frame.cpp:594-622"""
    vkps = []
    nbw = grid_width(P)[0]
    cs = F32(P["ncellsize"])
    rkp = int(np.floor(F32(kp["px"][1]) / cs))
    ckp = int(np.floor(F32(kp["px"][0]) / cs))
    for r in range(rkp - 1, rkp + 1):
        for c in range(ckp - 1, ckp + 1):
            idx = r * nbw + c
            if r < 0 or c < 0 or idx > len(frame["vgridkps_"]):
                continue
            if idx >= len(frame["vgridkps_"]):
                continue                                                # .at() would throw
            for kid in frame["vgridkps_"][idx]:
                if kid != kp["lmid"]:
                    if kid in frame["mapkps_"]:
                        vkps.append(frame["mapkps_"][kid])
    return vkps


def replay_stereo(P, frame, mps, ev=None):
    """MapManager::stereoMatching, :396-489 -> {lmid: (prior, has_prior, skip)}; has_prior 1: v3dpriors from the map point (:411),
    2: from the neighbours (:477); skip: the `continue` after removeMapPointObs (:416-417).  The SAD prior of the rectified branch
    (:422-437) is not part of this: it lives inside ov2_stereo_match."""
    out = {}
    T, Tr = pose(frame["Tcw"]), pose(P["Tcic0"])
    with np.errstate(all="ignore"):
        for lmid, kp in frame["mapkps_"].items():
            priorpt = kp["px"]
            if kp["is3d"]:
                plm = mps.get(kp["lmid"])
                if plm is not None:
                    projpt = project_dist(P, se3_act(Tr, se3_act(T, _w(plm))))
                    _margin(ev, P, projpt)
                    if in_image(P, projpt):
                        out[lmid] = (projpt, 1, 0)
                        continue
                else:
                    out[lmid] = (kp["px"], 0, 1)                        # removeMapPointObs(kp.lmid_, frame.kfid_)
                    continue
            if not P["rect"]:
                vnearkps = _surrounding(P, frame, kp)
                if len(vnearkps) >= 1:
                    vnear3dkps = [cokp for cokp in vnearkps if cokp["is3d"]]
                    if len(vnear3dkps) >= 1:
                        nb3dkp, mean_z, weights = 0, D(0), D(0)
                        for cokp in vnear3dkps:
                            plm = mps.get(cokp["lmid"])
                            if plm is not None:
                                nb3dkp += 1
                                coef = D(1) / pt_dist(cokp["unpx"], kp["unpx"])
                                weights = weights + coef
                                mean_z = mean_z + coef * se3_act(T, _w(plm))[2]
                        if nb3dkp >= 1:
                            mean_z = mean_z / weights
                            bv = _w(kp["bv"])
                            predcampt = tuple(mean_z * (b / bv[2]) for b in bv)
                            projpt = project_dist(P, se3_act(Tr, predcampt))
                            _margin(ev, P, projpt)
                            if in_image(P, projpt):
                                out[lmid] = (projpt, 2, 0)
                                continue
            out[lmid] = (priorpt, 0, 0)
    return out


# ---- the host's flattening ----------------------------------------------------------------------------------------------------------
def flatten(P, frame, mps):
    """the arrays of ov2_klt_priors_item and ov2_stereo_priors_item in one dict: keypoint rows in mapkps_ order, per cell the rows
    in vgridkps_ order"""
    ids = list(frame["mapkps_"].keys())
    row = {i: r for r, i in enumerate(ids)}
    kps = [frame["mapkps_"][i] for i in ids]
    n = len(ids)
    state = np.array([0 if not k["is3d"] else (1 if k["lmid"] in mps else 2) for k in kps], np.uint8).reshape(n)
    wpt = np.zeros((n, 3), np.float64)
    for r, k in enumerate(kps):
        if state[r] == 1:
            wpt[r] = mps[k["lmid"]]
    cell_start, cell_kp = [0], []
    for cell in frame["vgridkps_"]:
        cell_kp.extend(row[i] for i in cell if i in row)
        cell_start.append(len(cell_kp))
    return dict(Tcw=np.asarray(frame["Tcw"], np.float64), px=np.asarray([k["px"] for k in kps], np.float32).reshape(n, 2),
                unpx=np.asarray([k["unpx"] for k in kps], np.float32).reshape(n, 2),
                bv=np.asarray([k["bv"] for k in kps], np.float64).reshape(n, 3), wpt=wpt, state=state,
                is3d=np.array([1 if k["is3d"] else 0 for k in kps], np.uint8).reshape(n),
                cell_start=np.asarray(cell_start, np.int32), cell_kp=np.asarray(cell_kp, np.int32))


def klt_arrays(frame, res):
    ids = list(frame["mapkps_"].keys())
    return dict(prior=np.asarray([res[i][0] for i in ids], np.float32).reshape(len(ids), 2),
                has_prior=np.asarray([res[i][1] for i in ids], np.uint8).reshape(len(ids)))


def stereo_arrays(frame, res):
    ids = list(frame["mapkps_"].keys())
    out = klt_arrays(frame, res)
    out["skip"] = np.asarray([res[i][2] for i in ids], np.uint8).reshape(len(ids))
    return out


# ---- (b) the per-keypoint forms over the flattened arrays ----------------------------------------------------------------------------
def flat_klt(P, item, ev=None):
    """what ov2_klt_priors returns for (params, item)"""
    n = len(item["is3d"])
    out = dict(prior=np.array(item["px"], np.float32).reshape(n, 2), has_prior=np.zeros(n, np.uint8))
    T = pose(item["Tcw"])
    with np.errstate(all="ignore"):
        for i in range(n):
            if P["klt_use_prior"] and item["is3d"][i]:
                pr = project_dist(P, se3_act(T, _w(item["wpt"][i])))
                _margin(ev, P, pr)
                if in_image(P, pr):
                    out["prior"][i] = pr
                    out["has_prior"][i] = 1
    return out


def flat_stereo(P, item, ev=None):
    """what ov2_stereo_priors returns for (params, item)"""
    n = len(item["state"])
    out = dict(prior=np.array(item["px"], np.float32).reshape(n, 2), has_prior=np.zeros(n, np.uint8), skip=np.zeros(n, np.uint8))
    T, Tr = pose(item["Tcw"]), pose(P["Tcic0"])
    nbw, nbh = grid_width(P)
    cs = F32(P["ncellsize"])
    state, cell_start, cell_kp = item["state"], item["cell_start"], item["cell_kp"]
    with np.errstate(all="ignore"):
        for i in range(n):
            if state[i] == 2:
                out["skip"][i] = 1
                continue
            if state[i] == 1:
                pr = project_dist(P, se3_act(Tr, se3_act(T, _w(item["wpt"][i]))))
                _margin(ev, P, pr)
                if in_image(P, pr):
                    out["prior"][i] = pr
                    out["has_prior"][i] = 1
                    continue
            if P["rect"]:
                continue
            rf, cf = np.floor(F32(item["px"][i][1]) / cs), np.floor(F32(item["px"][i][0]) / cs)
            if not (abs(rf) <= 1048576. and abs(cf) <= 1048576.):
                continue
            rkp, ckp = int(rf), int(cf)
            nb, mean_z, weights = 0, D(0), D(0)
            for r in (rkp - 1, rkp):
                for c in (ckp - 1, ckp):
                    if r < 0 or c < 0 or r >= nbh or c >= nbw:
                        continue
                    idx = r * nbw + c
                    for k in cell_kp[cell_start[idx]:cell_start[idx + 1]]:
                        k = int(k)
                        if k == i or state[k] != 1:
                            continue
                        coef = D(1) / pt_dist(item["unpx"][k], item["unpx"][i])
                        weights = weights + coef
                        mean_z = mean_z + coef * se3_act(T, _w(item["wpt"][k]))[2]
                        nb += 1
            if nb == 0:
                if ev is not None:
                    ev["alone"] = ev.get("alone", 0) + 1
                continue
            mean_z = mean_z / weights
            if ev is not None and mean_z != mean_z:
                ev["nan_mean"] = ev.get("nan_mean", 0) + 1
            bv = _w(item["bv"][i])
            pr = project_dist(P, se3_act(Tr, tuple(mean_z * (b / bv[2]) for b in bv)))
            _margin(ev, P, pr)
            if in_image(P, pr):
                out["prior"][i] = pr
                out["has_prior"][i] = 2
    return out


def same(a, b, prior_ulp=0):
    """every field of two results equal bit for bit (NaN by mask); prior_ulp > 0 allows that many float ulps on prior"""
    for f in a:
        if f == "prior" or f.startswith("n_"):
            continue
        if f not in b or not np.array_equal(np.asarray(a[f]), np.asarray(b[f])):
            return False, f
    x, y = np.ascontiguousarray(a["prior"], np.float32), np.ascontiguousarray(b["prior"], np.float32)
    nx, ny = np.isnan(x), np.isnan(y)
    if x.shape != y.shape or not np.array_equal(nx, ny):
        return False, "prior"
    if prior_ulp:
        if not (np.abs(x[~nx].astype(np.float64) - y[~ny]) <= prior_ulp * np.spacing(np.abs(y[~ny]))).all():
            return False, "prior"
    elif not np.array_equal(x[~nx].view(np.uint32), y[~ny].view(np.uint32)):
        return False, "prior"
    return True, ""


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
def _bearing(P, u, v):
    fx, fy, cx, cy = P["K"]
    b = np.array([(u - cx) / fx, (v - cy) / fy, 1.0])
    return b / np.linalg.norm(b)


def make_scene(P, rng, n, p3d=0.6, pgone=0.12, pout=0.3):
    """(frame, mps): n keypoints spread over the image, a share p3d of them 3-D, pgone of those without their map point, pout of
    the rest with a map point that does not project where the keypoint is (behind the camera -- which projects INSIDE --, far to
    the side, nearly in the camera plane).  The grid cells list their keypoints in another order than mapkps_."""
    fx, fy, cx, cy = P["K"]
    W, H = P["img_w"], P["img_h"]
    nbw, nbh = grid_width(P)
    Tcw = _rand_pose(rng)
    mapkps, mps = {}, {}
    lmid = 100
    for _ in range(n):
        lmid += int(rng.integers(1, 5))
        u, v = rng.uniform(1, W - 1), rng.uniform(1, H - 1)                 # the undistorted pixel
        x, y = (u - cx) / fx, (v - cy) / fy
        px = project_dist(P, (D(x), D(y), D(1)))
        if not in_image(P, px):
            px = (F32(u), F32(v))
        is3d = rng.uniform() < p3d
        mapkps[lmid] = dict(lmid=lmid, px=px, unpx=(F32(u), F32(v)), bv=_bearing(P, u, v), is3d=bool(is3d))
        if not is3d or rng.uniform() < pgone:
            continue
        z = rng.uniform(2, 12)
        pc = np.array([x * z, y * z, z]) + rng.normal(0, 0.02, 3)
        if rng.uniform() < pout:
            kind = rng.uniform()
            if kind < 0.3:
                pc = -pc                                                    # behind the camera, same pixel
            elif kind < 0.8:
                pc[int(rng.integers(0, 2))] += rng.choice([-1, 1]) * rng.uniform(1.5, 5) * z
            else:
                pc[2] = rng.uniform(-0.01, 0.01)
        mps[lmid] = _inv_act(Tcw, pc)
    vgrid = [[] for _ in range(nbw * nbh)]
    ids = list(mapkps)
    cs = F32(P["ncellsize"])
    for j in rng.permutation(len(ids)):
        kp = mapkps[ids[j]]
        vgrid[int(np.floor(kp["px"][1] / cs)) * nbw + int(np.floor(kp["px"][0] / cs))].append(ids[j])
    return dict(Tcw=Tcw, mapkps_=mapkps, vgridkps_=vgrid), mps


SCENE_NS = (0, 1, 2, 63, 64, 65, 130, 308)
CAMERAS = (("pinhole", None), ("pinhole", RADTAN4), ("pinhole", RADTAN8), ("fisheye", FISHEYE4))


def scene_list(form):
    """[(name, P, frame, mps)]: every n of SCENE_NS with every camera of CAMERAS, rect / klt_use_prior alternating; form "klt": every
    3-D keypoint has its map point (map_plms_.at()), "stereo": some are gone"""
    out = []
    for ci, (model, Dv) in enumerate(CAMERAS):
        for ni, n in enumerate(SCENE_NS):
            flag = (ci + ni) % 2 == 0
            P = make_params(D=Dv, model=model, klt_use_prior=flag or n == 308, rect=not flag)
            rng = np.random.default_rng(7000 + 100 * ci + ni + (50 if form == "stereo" else 0))
            frame, mps = make_scene(P, rng, n, pgone=0.0 if form == "klt" else 0.15)
            out.append(("%s_%s%d_n%d" % (form, model, 0 if Dv is None else len(Dv), n), P, frame, mps))
    return out


# ---- crafted cases: one per quirk ---------------------------------------------------------------------------------------------------------
def toy(P, kps, Tcw=I7):
    """kps: [(lmid, px, state, wpt or None)]: unpx = px and bv from K (no distortion); state 2 = 3-D without a map point"""
    nbw, nbh = grid_width(P)
    vgrid = [[] for _ in range(nbw * nbh)]
    mapkps, mps = {}, {}
    for lmid, px, state, wpt in kps:
        px = (F32(px[0]), F32(px[1]))
        mapkps[lmid] = dict(lmid=lmid, px=px, unpx=px, bv=_bearing(P, float(px[0]), float(px[1])), is3d=state != 0)
        vgrid[int(px[1] // P["ncellsize"]) * nbw + int(px[0] // P["ncellsize"])].append(lmid)
        if state == 1:
            mps[lmid] = np.asarray(wpt, np.float64)
    return dict(Tcw=np.asarray(Tcw, np.float64), mapkps_=mapkps, vgridkps_=vgrid), mps


def at(P, u, v, z):
    """the camera-frame point at depth z on the ray of pixel (u, v)"""
    fx, fy, cx, cy = P["K"]
    return ((u - cx) / fx * z, (v - cy) / fy * z, z)


def crafted_klt():
    """[(name, P, frame, mps, expected has_prior list)]; identity pose, no distortion, K = (512, 512, 384, 256) on 768 x 512: the
    points (+-0.75, 0, 1) project exactly onto x = 768 and x = 0"""
    P = make_params(cam=CRAFT_CAM, Tcic0=I7)
    cases = []
    cases.append(("behind_camera_projects_inside", P, *toy(P, [(1, (300, 200), 1, (0.1, 0.1, -2.0))]), [1]))
    cases.append(("z_zero", P, *toy(P, [(1, (300, 200), 1, (0.0, 0.0, 0.0)), (2, (310, 200), 1, (1.0, 1.0, 0.0))]), [0, 0]))
    cases.append(("exactly_on_img_w_and_on_0", P, *toy(P, [(1, (300, 200), 1, (0.75, 0.0, 1.0)), (2, (310, 200), 1, (-0.75, 0.0, 1.0)),
                                                          (3, (320, 200), 1, (0.0, 0.5, 1.0)), (4, (330, 200), 1, (0.0, -0.5, 1.0))]),
                  [0, 1, 0, 1]))
    Pn = make_params(cam=CRAFT_CAM, Tcic0=I7, klt_use_prior=False)
    cases.append(("klt_use_prior_off", Pn, *toy(Pn, [(1, (300, 200), 1, at(Pn, 305, 203, 4.0)), (2, (10, 10), 0, None)]), [0, 0]))
    return cases


def crafted_stereo():
    """[(name, P, frame, mps, expected has_prior list, expected skip list)]; identity pose, the right camera 0.125 m to the right
    without rotation, no distortion: a point at depth z on the ray of (u, v) projects to (u - 64 / z, v) in the right image"""
    P = make_params(cam=CRAFT_CAM, Tcic0=(-0.125, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0))
    cases = []
    # A's map point lies far to the left of the right camera: its projection leaves the image, and the neighbour B gives the depth
    cases.append(("right_projection_leaves_then_neighbours", P,
                  *toy(P, [(1, (100, 100), 1, (-10.0, 0.0, 1.0)), (2, (105, 102), 1, at(P, 105, 102, 5.0))]), [2, 1], [0, 0]))
    # row 0 / column 0: r - 1 and c - 1 are skipped; the neighbour in the keypoint's own cell is found
    cases.append(("cell_row0_col0", P, *toy(P, [(1, (10, 10), 0, None), (2, (20, 12), 1, at(P, 20, 12, 16.0))]), [2, 1], [0, 0]))
    # column 0 of row 1: c - 1 = -1 is skipped, not wrapped into the last cell of row 0 (where keypoint 2 sits)
    cases.append(("column_minus_one_not_wrapped", P, *toy(P, [(1, (10, 40), 0, None), (2, (760, 10), 1, at(P, 760, 10, 4.0))]), [0, 1], [0, 0]))
    # alone in its 2 x 2 block: keypoint 2 is one cell to the right, which the block does not cover
    cases.append(("alone_in_block", P, *toy(P, [(1, (300, 200), 0, None), (2, (325, 200), 1, at(P, 325, 200, 4.0))]), [0, 1], [0, 0]))
    # a coincident unpx: coef = inf, mean_z = NaN, no prior -- although keypoint 3 alone would have given one
    cases.append(("coincident_unpx_nan", P, *toy(P, [(1, (300, 200), 0, None), (2, (300, 200), 1, at(P, 300, 200, 4.0)),
                                                    (3, (304, 203), 1, at(P, 304, 203, 4.0))]), [0, 1, 1], [0, 0, 0]))
    cases.append(("without_the_coincidence", P, *toy(P, [(1, (300, 200), 0, None), (3, (304, 203), 1, at(P, 304, 203, 4.0))]), [2, 1], [0, 0]))
    # a state-2 keypoint is skipped, and as the only neighbour of keypoint 1 it gives no depth; as state 1 it does
    cases.append(("state2_and_as_neighbour", P, *toy(P, [(1, (300, 200), 0, None), (2, (304, 203), 2, None)]), [0, 0], [0, 1]))
    cases.append(("state1_as_neighbour", P, *toy(P, [(1, (300, 200), 0, None), (2, (304, 203), 1, at(P, 304, 203, 4.0))]), [2, 1], [0, 0]))
    # exactly on 0 (inside) and exactly on img_w (outside, then no neighbour): x - 0.125 = -+0.75
    cases.append(("exactly_on_0_and_on_img_w", P, *toy(P, [(1, (300, 200), 1, (-0.625, 0.0, 1.0)), (2, (500, 400), 1, (0.875, 0.0, 1.0))]),
                  [1, 0], [0, 0]))
    Pr = make_params(cam=CRAFT_CAM, Tcic0=(-0.125, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0), rect=True)
    cases.append(("rect_stops_before_the_neighbours", Pr, *toy(Pr, [(1, (300, 200), 0, None), (2, (304, 203), 1, at(Pr, 304, 203, 4.0))]),
                  [0, 1], [0, 0]))
    return cases
