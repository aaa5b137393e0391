"""numpy restatement of the mapper's local-map matching (the reference's Mapper::matchToMap, src/mapper.cpp:576-774) as
include/ov2slam_hip.h specifies it for ov2_match_to_map, with Frame::getSurroundingKeypoints (src/frame.cpp:624-650),
CameraCalibration::projectCamToImageDist (src/camera_calibration.cpp:254-281) and MapPoint::computeMinDescDist.

Two independent forms:
  replay()    the reference loop statement by statement over a dict-based toy map (map points with set_kfids_ / map_kf_desc_,
              keyframes with mapkps_, the frame with mapkps_ / vgridkps_), `continue`s and the map clean-up included;
  flat()      the per-map-point form over the flattened arrays of ov2_match_keyframe, i.e. what k_map_match<false> (csrc/mapmatch.hip) computes.
flatten() turns a toy map into those arrays (what the host does before the call); tests/test_match_reference.py checks
replay == flat o flatten on every output field, bit for bit.

Arithmetic: np.float64 where the reference holds a double, np.float32 (`# f32`) where it holds a float; the Sophus / Eigen /
cv::norm conventions are those of tests/tri_ref.py.  view_th = cos(atan(.)) is taken in double and rounded to float per step.
The snapshot rule (header): a stale observation counts in the shared-observer test and is left out of the re-projection sum;
replay(mutate=True) also removes it from the map as the reference does, replay(mutate=False) is the documented deviation."""
import copy
import math

import numpy as np

from tests.tri_ref import D, F32, norm3, pose, pt_dist, se3_act

BEHIND, OUT_OF_FOV, OUT_OF_IMAGE, NO_CANDIDATE, RATIO_REJECTED, BEST = 1, 2, 4, 8, 16, 32
EUROC = dict(K=(458.654, 457.296, 367.215, 248.375), img_w=752, img_h=480, ncellsize=35)
RADTAN4 = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)
RADTAN5 = RADTAN4 + (-0.0091,)
FISHEYE4 = (-0.013721808247486035, 0.020727425669427896, -0.012786476702685545, 0.0025242267320687625)


def make_params(D=None, model="pinhole", cam=EUROC, fmax_proj_pxdist=2.0, fmax_desc_dist=0.2):
    return dict(model=model, K=tuple(cam["K"]), D=None if D is None else tuple(D), img_w=cam["img_w"], img_h=cam["img_h"],
                ncellsize=cam["ncellsize"], fmax_proj_pxdist=fmax_proj_pxdist, fmax_desc_dist=fmax_desc_dist)


# ---- the pieces both forms share: they are calls into other classes in the reference ------------------------------------------------
def thresholds(P, nb3dkps):
    """:586-602 and :650: (view_th, dmaxpxdist, mindist), floats"""
    fx, fy = D(P["K"][0]), D(P["K"][1])
    vfov = F32(D(0.5) * D(P["img_h"]) / fy)                             # f32
    hfov = F32(D(0.5) * D(P["img_w"]) / fx)                             # f32
    maxradfov = F32(math.atan(float(hfov if hfov > vfov else vfov)))    # f32
    view_th = F32(math.cos(float(maxradfov)))                           # f32
    dmax = F32(P["fmax_proj_pxdist"])
    if nb3dkps < 30:
        dmax = F32(D(dmax) * D(2))                                      # f32 *= 2.
    mindist = F32(D(F32(32) * F32(P["fmax_desc_dist"])) * D(8))         # int * float, * 8., stored to float
    return view_th, dmax, mindist


def grid_width(P):
    """Frame's nbwcells_ / nbhcells_ (frame.cpp:41-42)"""
    c = F32(P["ncellsize"])
    return int(np.ceil(F32(P["img_w"]) / c)), int(np.ceil(F32(P["img_h"]) / c))


def distort(P, x, y):
    """the forward model on normalised coordinates (doubles) -> pixel (doubles), in the published operation order"""
    fx, fy, cx, cy = (D(v) for v in P["K"])
    k = [D(v) for v in P["D"]] + [D(0)] * (12 - len(P["D"]))
    one = D(1)
    if P.get("model", "pinhole") == "fisheye":
        r = np.sqrt(x * x + y * y)
        th = D(math.atan(float(r)))
        th2 = th * th; th4 = th2 * th2; th6 = th4 * th2; th8 = th4 * th4
        thd = th * (one + k[0] * th2 + k[1] * th4 + k[2] * th6 + k[3] * th8)
        cdist = thd * (one / r) if r > 1e-8 else one
        return (x * cdist) * fx + cx, (y * cdist) * fy + cy
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = k
    r2 = x * x + y * y; r4 = r2 * r2; r6 = r4 * r2
    a1 = D(2) * x * y; a2 = r2 + D(2) * x * x; a3 = r2 + D(2) * y * y
    cdist = one + k1 * r2 + k2 * r4 + k3 * r6
    icdist2 = one / (one + k4 * r2 + k5 * r4 + k6 * r6)
    xd = x * cdist * icdist2 + p1 * a1 + p2 * a2 + s1 * r2 + s2 * r4
    yd = y * cdist * icdist2 + p1 * a3 + p2 * a1 + s3 * r2 + s4 * r4
    return xd * fx + cx, yd * fy + cy


def project_dist(P, p):
    """CameraCalibration::projectCamToImageDist: cv::Point2f"""
    with np.errstate(all="ignore"):
        fx, fy, cx, cy = (D(v) for v in P["K"])
        invz = D(1) / D(p[2])
        x, y = D(p[0]) * invz, D(p[1]) * invz
        if not P.get("D"):
            return (F32(fx * x + cx), F32(fy * y + cy))                 # f32
        u, v = distort(P, D(F32(x)), D(F32(y)))                         # f32: cv::Point3f / Point2f
        return (F32(u), F32(v))                                         # f32


def in_image(P, px):
    """Frame::isInImage: float against the double img_w_ / img_h_"""
    return bool(px[0] >= 0 and px[1] >= 0 and D(px[0]) < D(P["img_w"]) and D(px[1]) < D(P["img_h"]))


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(np.asarray(a, np.uint8), np.asarray(b, np.uint8))).sum())


def _ev(ev, key, n=1):
    if ev is not None:
        ev[key] = ev.get(key, 0) + n


def _margin(ev, *vals):
    """smallest distance of a gate quantity from its threshold met so far (the fisheye scenes are filtered on it)"""
    if ev is not None:
        for v in vals:
            v = abs(float(v))
            if v == v:
                ev["margin"] = min(ev.get("margin", np.inf), v)


# ---- (a) the reference loop, literally, over the toy map ----------------------------------------------------------------------------
def replay(M, mutate=True, ev=None):
    """Mapper::matchToMap(frame, fmaxprojerr, fdistratio, set_local_lmids).  M: params, frame (kfid_, Tcw, nb3dkps_, mapkps_
    {lmid: px_}, vgridkps_ [cell][...] of keypoint ids), mps {lmid: is3d_, wpt, set_kfids_, map_kf_desc_ {kfid: 32 bytes}},
    kfs {kfid: Tcw, mapkps_ {lmid: px_}}, local [lmid ...] (the iteration order of set_local_lmids).
    Returns (map_previd_newid, diag) with diag[lmid] = (status, bestid, bestdist, projpx) for every local id that got past the
    host-side filters (:613-623)."""
    P, frame, mps, kfs = M["params"], M["frame"], M["mps"], M["kfs"]
    map_previd_newid, diag = {}, {}
    if not M["local"]:
        return map_previd_newid, diag
    view_th, dmaxpxdist, _ = thresholds(P, frame["nb3dkps_"])
    nbwcells = grid_width(P)[0]
    Tcw = pose(frame["Tcw"])
    map_kpids_vlmidsdist = {}
    for lmid in M["local"]:
        if lmid in frame["mapkps_"]:                                    # frame.isObservingKp(lmid)
            continue
        plm = mps.get(lmid)
        if plm is None:
            continue
        elif not plm["is3d_"] or not plm["map_kf_desc_"]:
            continue
        wpt = tuple(D(v) for v in plm["wpt"])
        campt = se3_act(Tcw, wpt)
        if campt[2] < 0.1:
            diag[lmid] = (BEHIND, -1, F32(0), (F32(0), F32(0)))
            continue
        with np.errstate(all="ignore"):
            view_angle = F32(campt[2] / norm3(campt))                   # f32
        if abs(view_angle) < view_th:
            diag[lmid] = (OUT_OF_FOV, -1, F32(0), (F32(0), F32(0)))
            continue
        projpx = project_dist(P, campt)
        if not in_image(P, projpx):
            diag[lmid] = (OUT_OF_IMAGE, -1, F32(0), projpx)
            continue
        _margin(ev, projpx[0], projpx[1], D(projpx[0]) - D(P["img_w"]), D(projpx[1]) - D(P["img_h"]))
        # frame.getSurroundingKeypoints(projpx)
        vnearkps = []
        cs = F32(P["ncellsize"])
        rkp = int(np.floor(projpx[1] / cs))
        ckp = int(np.floor(projpx[0] / cs))
        _margin(ev, projpx[1] - F32(rkp) * cs, projpx[0] - F32(ckp) * cs, projpx[1] - F32(rkp + 1) * cs, projpx[0] - F32(ckp + 1) * cs)
        for r in range(rkp - 1, rkp + 1):
            for c in range(ckp - 1, ckp + 1):
                idx = r * nbwcells + c
                if r < 0 or c < 0 or idx > len(frame["vgridkps_"]):
                    continue
                for kid in frame["vgridkps_"][idx]:
                    if kid in frame["mapkps_"]:
                        vnearkps.append((kid, frame["mapkps_"][kid]))
        mindist = thresholds(P, frame["nb3dkps_"])[2]
        bestid, secid = -1, -1
        bestdist, secdist = mindist, mindist
        for kp_lmid, kp_px in vnearkps:
            if kp_lmid < 0:
                continue
            pxdist = F32(pt_dist(projpx, kp_px))                        # f32
            _margin(ev, D(pxdist) - D(dmaxpxdist))
            if pxdist > dmaxpxdist:
                _ev(ev, "gate_pxdist")
                continue
            pkplm = mps.get(kp_lmid)
            if pkplm is None:
                continue                                                # removeMapPointObs(kp.lmid_, frame.kfid_): the frame's own keypoint, host side
            if not pkplm["map_kf_desc_"]:
                continue
            is_candidate = True
            set_plmkfs = set(plm["set_kfids_"])
            for kfid in sorted(pkplm["set_kfids_"]):
                if kfid in set_plmkfs:
                    is_candidate = False
                    break
            if not is_candidate:
                _ev(ev, "gate_shared")
                continue
            coprojpx = F32(0)
            nbcokp = 0
            for kfid in sorted(pkplm["set_kfids_"]):
                pcokf = kfs.get(kfid)
                if pcokf is not None:
                    if kp_lmid in pcokf["mapkps_"]:                     # cokp.lmid_ == kp.lmid_
                        d = pt_dist(pcokf["mapkps_"][kp_lmid], project_dist(P, se3_act(pose(pcokf["Tcw"]), wpt)))
                        with np.errstate(all="ignore"):
                            coprojpx = F32(D(coprojpx) + d)             # f32 += double
                        nbcokp += 1
                    elif mutate:
                        _remove_obs(pkplm, kfid)
                elif mutate:
                    _remove_obs(pkplm, kfid)
            with np.errstate(all="ignore"):
                mean = coprojpx / F32(nbcokp)                           # 0 / 0: NaN, the comparison is false
            _margin(ev, D(mean) - D(dmaxpxdist))
            if mean > dmaxpxdist:
                _ev(ev, "gate_coproj")
                continue
            dist = _min_desc_dist(plm, pkplm)
            if dist <= bestdist:
                if bestid != -1 and dist == bestdist:
                    _ev(ev, "tie_best")
                secdist, secid = bestdist, bestid
                bestdist, bestid = dist, kp_lmid
            elif dist <= secdist:
                secdist, secid = dist, kp_lmid
        status = BEST
        if bestid != -1 and secid != -1:
            if D(0.9) * D(secdist) < D(bestdist):
                bestid = -1
                status = RATIO_REJECTED
        elif bestid == -1:
            status = NO_CANDIDATE
        diag[lmid] = (status, bestid, bestdist, projpx)
        if bestid < 0:
            continue
        map_kpids_vlmidsdist.setdefault(bestid, []).append((lmid, bestdist))
    kp_dist = {}
    for kpid in sorted(map_kpids_vlmidsdist):
        bestdist, bestlmid = F32(1024), -1
        for lmid, d in map_kpids_vlmidsdist[kpid]:
            if d <= bestdist:
                if bestlmid >= 0 and d == bestdist:
                    _ev(ev, "tie_pick")
                bestdist, bestlmid = d, lmid
        if bestlmid >= 0:
            map_previd_newid[kpid] = bestlmid
            kp_dist[kpid] = bestdist
    diag["kp_dist"] = kp_dist
    return map_previd_newid, diag


def _remove_obs(mp, kfid):
    """MapManager::removeMapPointObs -> MapPoint::removeKfObs: the observer and its descriptor leave the map point"""
    mp["set_kfids_"] = [k for k in mp["set_kfids_"] if k != kfid]
    mp["map_kf_desc_"].pop(kfid, None)


def _min_desc_dist(a, b):
    """MapPoint::computeMinDescDist (src/map_point.cpp:236-252)"""
    min_dist = F32(1000)
    for d1 in a["map_kf_desc_"].values():
        for d2 in b["map_kf_desc_"].values():
            dist = F32(hamming(d1, d2))
            if dist < min_dist:
                min_dist = dist
    return min_dist


# ---- the host's flattening -------------------------------------------------------------------------------------------------------------
def flatten(M):
    """(kf, meta): the arrays of ov2_match_keyframe for the toy map, and meta = dict(kp_lmid, lm_lmid) to map rows back to ids.
    Map-point rows: ascending lmid; pose rows: ascending kfid; keypoint rows: the order of frame.mapkps_."""
    P, frame, mps, kfs = M["params"], M["frame"], M["mps"], M["kfs"]
    kp_lmid = list(frame["mapkps_"].keys())
    lm_lmid = [i for i in M["local"] if i not in frame["mapkps_"] and i in mps and mps[i]["is3d_"] and mps[i]["map_kf_desc_"]]
    rows = sorted(set(lm_lmid) | {i for i in kp_lmid if i in mps and mps[i]["map_kf_desc_"]})
    row_of = {i: r for r, i in enumerate(rows)}
    kfids = sorted(kfs)
    kf_row = {k: r for r, k in enumerate(kfids)}
    obs_start, obs_kfid, obs_kf, obs_px, desc_start, desc = [0], [], [], [], [0], []
    for i in rows:
        for k in sorted(mps[i]["set_kfids_"]):
            ok = k in kfs and i in kfs[k]["mapkps_"]
            obs_kfid.append(k); obs_kf.append(kf_row[k] if ok else -1)
            obs_px.append(kfs[k]["mapkps_"][i] if ok else (0, 0))
        obs_start.append(len(obs_kfid))
        desc.extend(mps[i]["map_kf_desc_"].values())
        desc_start.append(len(desc))
    kp_row = {i: r for r, i in enumerate(kp_lmid)}
    cell_start, cell_kp = [0], []
    nbw, nbh = grid_width(P)
    for c in range(nbw * nbh):
        cell_kp.extend(kp_row[i] for i in frame["vgridkps_"][c] if i in kp_row)
        cell_start.append(len(cell_kp))
    kf = dict(Tcw=np.asarray(frame["Tcw"], np.float64), nb3dkps=int(frame["nb3dkps_"]),
              kp_px=np.asarray([frame["mapkps_"][i] for i in kp_lmid], np.float32).reshape(-1, 2),
              kp_mp=np.asarray([row_of.get(i, -1) if i >= 0 else -1 for i in kp_lmid], np.int32),
              cell_start=np.asarray(cell_start, np.int32), cell_kp=np.asarray(cell_kp, np.int32),
              obs_start=np.asarray(obs_start, np.int32), obs_kfid=np.asarray(obs_kfid, np.int32),
              obs_kf=np.asarray(obs_kf, np.int32), obs_px=np.asarray(obs_px, np.float32).reshape(-1, 2),
              desc_start=np.asarray(desc_start, np.int32), desc=np.asarray(desc, np.uint8).reshape(-1, 32),
              kf_Tcw=np.asarray([kfs[k]["Tcw"] for k in kfids], np.float64).reshape(-1, 7),
              lm_mp=np.asarray([row_of[i] for i in lm_lmid], np.int32),
              lm_wpt=np.asarray([mps[i]["wpt"] for i in lm_lmid], np.float64).reshape(-1, 3))
    return kf, dict(kp_lmid=kp_lmid, lm_lmid=lm_lmid)


def replay_arrays(M, meta, mutate=True, ev=None):
    """replay() in the layout of flat()'s result"""
    prev_new, diag = replay(copy.deepcopy(M), mutate=mutate, ev=ev)
    kp_row = {i: r for r, i in enumerate(meta["kp_lmid"])}
    lm_row = {i: r for r, i in enumerate(meta["lm_lmid"])}
    out = _empty(len(meta["lm_lmid"]), len(meta["kp_lmid"]))
    for l, lmid in enumerate(meta["lm_lmid"]):
        st, bestid, bestdist, px = diag[lmid]
        out["lm_status"][l] = st
        out["lm_kp"][l] = kp_row[bestid] if st == BEST else -1
        out["lm_dist"][l] = bestdist
        out["lm_projpx"][l] = px
    for kpid, lmid in prev_new.items():
        out["kp_lm"][kp_row[kpid]] = lm_row[lmid]
        out["kp_dist"][kp_row[kpid]] = diag["kp_dist"][kpid]
    out["n_matches"] = len(prev_new)
    return out


def _empty(n_lm, n_kp):
    return dict(lm_status=np.zeros(n_lm, np.uint8), lm_kp=np.full(n_lm, -1, np.int32), lm_dist=np.zeros(n_lm, np.float32),
                lm_projpx=np.zeros((n_lm, 2), np.float32), kp_lm=np.full(n_kp, -1, np.int32), kp_dist=np.zeros(n_kp, np.float32),
                n_matches=0)


# ---- (b) the per-map-point form over the flattened arrays ----------------------------------------------------------------------------
def flat(P, kf, ev=None):
    """what ov2_match_to_map returns for (params, keyframe): a dict of the arrays of ov2_match_result"""
    view_th, dmax, mindist = thresholds(P, kf["nb3dkps"])
    nbw = grid_width(P)[0]
    cs = F32(P["ncellsize"])
    T = pose(kf["Tcw"])
    obs_start, desc_start, cell_start = kf["obs_start"], kf["desc_start"], kf["cell_start"]
    n_lm, n_kp = len(kf["lm_mp"]), len(kf["kp_mp"])
    out = _empty(n_lm, n_kp)
    proposals = [[] for _ in range(n_kp)]
    for l in range(n_lm):
        w = tuple(D(v) for v in kf["lm_wpt"][l])
        A = int(kf["lm_mp"][l])
        cp = se3_act(T, w)
        if cp[2] < 0.1:
            out["lm_status"][l] = BEHIND
            continue
        with np.errstate(all="ignore"):
            va = F32(cp[2] / norm3(cp))                                 # f32
        if abs(va) < view_th:
            out["lm_status"][l] = OUT_OF_FOV
            continue
        px = project_dist(P, cp)
        out["lm_projpx"][l] = px
        if not in_image(P, px):
            out["lm_status"][l] = OUT_OF_IMAGE
            continue
        _margin(ev, px[0], px[1], D(px[0]) - D(P["img_w"]), D(px[1]) - D(P["img_h"]))
        rkp, ckp = int(np.floor(px[1] / cs)), int(np.floor(px[0] / cs))
        _margin(ev, px[1] - F32(rkp) * cs, px[0] - F32(ckp) * cs, px[1] - F32(rkp + 1) * cs, px[0] - F32(ckp + 1) * cs)
        idsA = set(int(v) for v in kf["obs_kfid"][obs_start[A]:obs_start[A + 1]])
        descA = kf["desc"][desc_start[A]:desc_start[A + 1]]
        bestid, secid, bestdist, secdist = -1, -1, mindist, mindist
        for r in (rkp - 1, rkp):
            for c in (ckp - 1, ckp):
                if r < 0 or c < 0:
                    continue
                idx = r * nbw + c
                for k in kf["cell_kp"][cell_start[idx]:cell_start[idx + 1]]:
                    k = int(k)
                    B = int(kf["kp_mp"][k])
                    if B < 0:
                        continue
                    descB = kf["desc"][desc_start[B]:desc_start[B + 1]]
                    if len(descB) == 0:
                        continue
                    pxdist = F32(pt_dist(px, kf["kp_px"][k]))           # f32
                    _margin(ev, D(pxdist) - D(dmax))
                    if pxdist > dmax:
                        _ev(ev, "gate_pxdist")
                        continue
                    o0, o1 = int(obs_start[B]), int(obs_start[B + 1])
                    if any(int(v) in idsA for v in kf["obs_kfid"][o0:o1]):
                        _ev(ev, "gate_shared")
                        continue
                    co, nco = F32(0), 0
                    for j in range(o0, o1):                             # ascending keyframe id
                        row = int(kf["obs_kf"][j])
                        if row < 0:
                            continue
                        d = pt_dist(kf["obs_px"][j], project_dist(P, se3_act(pose(kf["kf_Tcw"][row]), w)))
                        with np.errstate(all="ignore"):
                            co = F32(D(co) + d)                         # f32 += double
                        nco += 1
                    with np.errstate(all="ignore"):
                        mean = co / F32(nco)
                    _margin(ev, D(mean) - D(dmax))
                    if mean > dmax:
                        _ev(ev, "gate_coproj")
                        continue
                    _ev(ev, "compared")
                    hm = 1000
                    if len(descA):
                        x = np.bitwise_xor(descA[:, None, :], descB[None, :, :])
                        hm = min(hm, int(np.unpackbits(x, axis=2).sum(axis=2).min()))
                    dist = F32(hm)
                    if dist <= bestdist:
                        if bestid != -1 and dist == bestdist:
                            _ev(ev, "tie_best")
                        secdist, secid, bestdist, bestid = bestdist, bestid, dist, k
                    elif dist <= secdist:
                        secdist, secid = dist, k
        out["lm_dist"][l] = bestdist
        if bestid == -1:
            out["lm_status"][l] = NO_CANDIDATE
        elif secid != -1 and D(0.9) * D(secdist) < D(bestdist):
            out["lm_status"][l] = RATIO_REJECTED
        else:
            out["lm_status"][l] = BEST
            out["lm_kp"][l] = bestid
            proposals[bestid].append((l, bestdist))
    for k in range(n_kp):
        best, bl = F32(1024), -1
        for l, d in proposals[k]:
            if d <= best:
                if bl >= 0 and d == best:
                    _ev(ev, "tie_pick")
                best, bl = d, l
        if bl >= 0:
            out["kp_lm"][k], out["kp_dist"][k] = bl, best
            out["n_matches"] += 1
    return out


def same(a, b, projpx_ulp=0):
    """every field of two results equal bit for bit (NaN by mask); projpx_ulp > 0 allows that many float ulps on lm_projpx"""
    for f in ("lm_status", "lm_kp", "kp_lm"):
        if not np.array_equal(a[f], b[f]):
            return False, f
    for f in ("lm_dist", "kp_dist", "lm_projpx"):
        x, y = np.ascontiguousarray(a[f], np.float32), np.ascontiguousarray(b[f], np.float32)
        nx, ny = np.isnan(x), np.isnan(y)
        if x.shape != y.shape or not np.array_equal(nx, ny):
            return False, f
        if f == "lm_projpx" and projpx_ulp:
            if not (np.abs(x[~nx].astype(np.float64) - y[~ny]) <= projpx_ulp * np.spacing(np.abs(y[~ny]))).all():
                return False, f
        elif not np.array_equal(x[~nx].view(np.uint32), y[~ny].view(np.uint32)):
            return False, f
    return (int(a["n_matches"]) == int(b["n_matches"])), "n_matches"


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------
def _quat(rng, s):
    v = rng.normal(0, s, 3)
    q = np.array([v[0], v[1], v[2], 1.0])
    return q / np.linalg.norm(q)


def _rand_pose(rng, rot=0.05, trans=0.3):
    return np.concatenate([rng.normal(0, trans, 3), _quat(rng, rot)])


def _inv_act(T, pc):
    """world point whose camera-frame image under T (= Tcw) is pc (float64 algebra: the generator only needs to be close)"""
    t, q = np.asarray(T[:3], np.float64), np.asarray(T[3:], np.float64)
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return R.T @ (np.asarray(pc, np.float64) - t)


def _flip(rng, d, nbits):
    d = np.array(d, np.uint8)
    for b in rng.choice(256, size=nbits, replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def make_scene(P, rng, *, n_kp=120, n_lm=260, n_kf=8, nb3dkps=100, dup=0.5, many_obs=0, max_obs=4):
    """A toy map around one new keyframe.  Keypoints carry map points seen from a few of n_kf keyframes; the local map holds
    planted duplicates of those map points (re-detections a few descriptor bits away, seen from OTHER keyframes), twins that trip
    the ratio test, exact descriptor ties, pairs that propose the same keypoint, points that share an observer with their
    candidate, points moved along the viewing ray (the re-projection gate), and points spread over and around the field of view.
    many_obs: that many keypoint map points get up to 80 observers (n_kf is raised to 90)."""
    if many_obs:
        n_kf = max(n_kf, 90)
    fx, fy, cx, cy = P["K"]
    W, H, cell = P["img_w"], P["img_h"], P["ncellsize"]
    nbw, nbh = grid_width(P)
    Tcw = _rand_pose(rng)
    kfids = sorted(int(v) for v in rng.choice(400, size=n_kf, replace=False))
    new_kfid = 500
    kfs = {k: dict(Tcw=_rand_pose(rng), mapkps_={}) for k in kfids}
    mps, frame_kps, vgrid = {}, {}, [[] for _ in range(nbw * nbh)]
    next_id = [1000]

    def new_id():
        next_id[0] += int(rng.integers(1, 4))
        return next_id[0]

    def observe(lmid, wpt, ks, noise):
        for k in ks:
            px = project_dist(P, se3_act(pose(kfs[k]["Tcw"]), tuple(D(v) for v in wpt)))
            kfs[k]["mapkps_"][lmid] = (F32(px[0] + F32(rng.normal(0, noise))), F32(px[1] + F32(rng.normal(0, noise))))

    def add_mp(wpt, ks, base, bits=3, noise=0.3, is3d=True):
        lmid = new_id()
        mps[lmid] = dict(is3d_=is3d, wpt=np.asarray(wpt, np.float64), set_kfids_=sorted(ks),
                         map_kf_desc_={k: _flip(rng, base, int(rng.integers(0, bits + 1))) for k in ks})
        observe(lmid, wpt, ks, noise)
        return lmid

    def add_kp(pc, ks, base, px_off=(0.0, 0.0)):
        """a keypoint of the new keyframe at the projection of camera-frame point pc (+ px_off), with its own map point"""
        px = project_dist(P, tuple(D(v) for v in pc))
        px = (F32(px[0] + F32(px_off[0])), F32(px[1] + F32(px_off[1])))
        if not in_image(P, px):
            return None
        wpt = _inv_act(Tcw, pc)
        lmid = add_mp(wpt, ks, base)
        mps[lmid]["set_kfids_"] = sorted(ks + [new_kfid])              # the new keyframe observes it (it is not in the pose table's re-projections: flatten marks what the map lacks)
        mps[lmid]["map_kf_desc_"][new_kfid] = _flip(rng, base, 1)
        frame_kps[lmid] = px
        vgrid[int(np.floor(px[1] / F32(cell))) * nbw + int(np.floor(px[0] / F32(cell)))].append(lmid)
        return lmid

    kfs[new_kfid] = dict(Tcw=Tcw, mapkps_={})                           # the new keyframe is in the map already (addKeyframe precedes the mapper)
    local, planted = [], []
    for i in range(n_kp):
        z = rng.uniform(2, 12)
        u, v = rng.uniform(8, W - 8), rng.uniform(8, H - 8)
        pc = np.array([(u - cx) / fx * z, (v - cy) / fy * z, z])
        nobs = int(rng.integers(1, max_obs + 1))
        if i < many_obs:
            nobs = int(rng.integers(66, 81))
        ks = [int(k) for k in rng.choice(kfids, size=nobs, replace=False)]
        base = rng.integers(0, 256, 32).astype(np.uint8)
        b = add_kp(pc, ks, base)
        if b is None:
            continue
        kfs[new_kfid]["mapkps_"][b] = frame_kps[b]
        kind = rng.uniform()
        if kind > dup:
            continue
        others = [k for k in kfids if k not in ks]
        if not others:
            continue
        oks = [int(k) for k in rng.choice(others, size=min(len(others), int(rng.integers(1, 4))), replace=False)]
        wpt = _inv_act(Tcw, pc + rng.normal(0, 0.002, 3))
        sub = rng.uniform()
        if sub < 0.45:                                                  # a plain duplicate
            planted.append((add_mp(wpt, oks, base), b)); local.append(planted[-1][0])
        elif sub < 0.55:                                                # shares an observer with its candidate
            local.append(add_mp(wpt, oks + ks[:1], base))
        elif sub < 0.65:                                                # moved along the viewing ray: same pixel here, elsewhere not
            local.append(add_mp(_inv_act(Tcw, pc * rng.uniform(1.3, 1.8)), oks, base))
        elif sub < 0.80:                                                # a twin keypoint 1 px away with nearly the same descriptor: ratio test
            t = add_kp(pc, ks, base, px_off=(1.0, 0.5))
            if t is not None:
                kfs[new_kfid]["mapkps_"][t] = frame_kps[t]
            local.append(add_mp(wpt, oks, _flip(rng, base, 16), bits=1))   # ~16 bits from both: second best within 10 % of the best
        elif sub < 0.88:                                                # exact descriptor tie between two candidates
            t = add_kp(pc, ks, base, px_off=(-0.75, 0.5))
            a = add_mp(wpt, oks, base, bits=0)
            for m in (b, t):
                if m is not None:
                    mps[m]["map_kf_desc_"][ks[0]] = np.array(base, np.uint8)
            if t is not None:
                kfs[new_kfid]["mapkps_"][t] = frame_kps[t]
            local.append(a)
        else:                                                           # two local points propose the same keypoint, at equal distance or not
            a1 = add_mp(wpt, oks, base, bits=0)
            a2 = add_mp(_inv_act(Tcw, pc + rng.normal(0, 0.002, 3)), oks, base, bits=0 if rng.uniform() < 0.5 else 4)
            mps[b]["map_kf_desc_"][ks[0]] = _flip(rng, base, 2)
            planted.append((a1, b))
            local += [a1, a2]
    while len(local) < n_lm:                                            # the rest of the local map: all around the camera
        kind = rng.uniform()
        z = rng.uniform(0.5, 15)
        if kind < 0.15:
            pc = np.array([rng.normal(0, 2), rng.normal(0, 2), rng.uniform(-5, 0.09)])
        elif kind < 0.5:
            pc = np.array([rng.uniform(-1.6, 1.6) * z, rng.uniform(-1.2, 1.2) * z, z])
        else:
            u, v = rng.uniform(0, W), rng.uniform(0, H)
            pc = np.array([(u - cx) / fx * z, (v - cy) / fy * z, z])
        ks = [int(k) for k in rng.choice(kfids, size=int(rng.integers(1, max_obs + 1)), replace=False)]
        local.append(add_mp(_inv_act(Tcw, pc), ks, rng.integers(0, 256, 32).astype(np.uint8), is3d=rng.uniform() > 0.03))
    taken = {b for _, b in planted}
    for lmid in list(frame_kps):                                        # keypoints whose map point is gone, or holds no descriptor
        if lmid not in taken and rng.uniform() < 0.06:
            if rng.uniform() < 0.5:
                del mps[lmid]
            else:
                mps[lmid]["map_kf_desc_"] = {}
    order = rng.permutation(len(local))
    local = [local[i] for i in order]
    local += list(frame_kps)[:3] + [999999]                             # ids the host filters: observed by the frame, unknown
    frame = dict(kfid_=new_kfid, Tcw=Tcw, nb3dkps_=nb3dkps, mapkps_=frame_kps, vgridkps_=vgrid)
    return dict(params=P, frame=frame, mps=mps, kfs=kfs, local=local, planted=planted)


def filtered_scene(P, seed, min_margin=1e-3, **kw):
    """make_scene, resampled until no gate quantity of the reference form lies within min_margin px of its threshold"""
    for t in range(200):
        M = make_scene(P, np.random.default_rng(1000 * seed + t), **kw)
        kf, meta = flatten(M)
        ev = {}
        ref = flat(P, kf, ev)
        if ev.get("margin", np.inf) >= min_margin:
            return M, kf, meta, ref
    raise RuntimeError("no scene with the requested margin")


# ---- crafted cases: one per quirk ---------------------------------------------------------------------------------------------------------
CRAFT_CAM = dict(K=(400.0, 400.0, 376.0, 240.0), img_w=752, img_h=480, ncellsize=35)
_I7 = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)


def _toy(P, kps, local, kfs, nb3dkps=100):
    """kps: [(lmid, px, kfids, descs) or (lmid, px, None)] (None: the keypoint's map point is gone); local: [(lmid, wpt, kfids,
    descs)]; kfs: {kfid: (Tcw, {lmid: px})}.  The frame's pose is the identity: camera frame = world frame."""
    nbw, nbh = grid_width(P)
    vgrid = [[] for _ in range(nbw * nbh)]
    mps, mapkps = {}, {}
    for kp in kps:
        lmid, px = kp[0], (F32(kp[1][0]), F32(kp[1][1]))
        mapkps[lmid] = px
        vgrid[int(px[1] // P["ncellsize"]) * nbw + int(px[0] // P["ncellsize"])].append(lmid)
        if kp[2] is not None:
            mps[lmid] = dict(is3d_=True, wpt=np.zeros(3), set_kfids_=sorted(kp[2]), map_kf_desc_=dict(zip(range(900, 999), kp[3])))
    for lmid, wpt, ks, descs in local:
        mps[lmid] = dict(is3d_=True, wpt=np.asarray(wpt, np.float64), set_kfids_=sorted(ks), map_kf_desc_=dict(zip(range(900, 999), descs)))
    K = {k: dict(Tcw=np.asarray(v[0], np.float64), mapkps_={i: (F32(p[0]), F32(p[1])) for i, p in v[1].items()}) for k, v in kfs.items()}
    frame = dict(kfid_=77, Tcw=np.asarray(_I7), nb3dkps_=nb3dkps, mapkps_=mapkps, vgridkps_=vgrid)
    return dict(params=P, frame=frame, mps=mps, kfs=K, local=[l[0] for l in local], planted=[])


def _at(P, u, v, z=4.0):
    fx, fy, cx, cy = P["K"]
    return ((u - cx) / fx * z, (v - cy) / fy * z, z)


def crafted_cases():
    """[(name, M, expected lm_status list, expected lm_kp list or None)]; the frame's pose is the identity and there is no
    distortion, so a point built with _at() projects onto the pixel it names (to float rounding)"""
    P = make_params(cam=CRAFT_CAM)
    d0 = np.arange(32, dtype=np.uint8)
    d1 = d0.copy(); d1[0] ^= 1
    cases = []
    # the 2x2 block: cells {rkp-1, rkp} x {ckp-1, ckp}.  104.5 is in column 2 (70..105); a keypoint at 105.5 (column 3) is 1 px
    # away and not seen; from 105.2 (column 3) the same keypoint is seen
    cases.append(("block_2x2_misses_right_cell", _toy(P, [(1, (105.5, 100.0), [], [d0])],
                                                      [(10, _at(P, 104.5, 100.0), [3], [d1]), (11, _at(P, 105.25, 100.0), [3], [d1])], {}),
                  [NO_CANDIDATE, BEST], [-1, 0]))
    # c = -1 is skipped, not wrapped into the previous row's last cell: with a 2000 px radius the keypoint there would match
    # (fy = 200 widens the viewing cone to the vertical half-angle, so the image's left edge is inside it)
    Pw = make_params(cam=dict(CRAFT_CAM, K=(400.0, 200.0, 376.0, 240.0)), fmax_proj_pxdist=2000.0)
    cases.append(("column_minus_one_skipped", _toy(Pw, [(1, (745.0, 50.0), [], [d0])], [(10, _at(Pw, 10.0, 100.0), [3], [d1])], {}),
                  [NO_CANDIDATE], [-1]))
    # the candidate's map point has no observer at all: 0 / 0 is NaN, the comparison is false, it passes
    cases.append(("nbcokp_zero_passes", _toy(P, [(1, (300.0, 200.0), [], [d0])], [(10, _at(P, 300.5, 200.0), [3], [d1])], {}),
                  [BEST], [0]))
    # 3 px away with fmax_proj_pxdist = 2: inside the doubled radius below 30 3-D keypoints only
    for nb, st, kp in ((29, BEST, 0), (30, NO_CANDIDATE, -1)):
        cases.append(("radius_nb3dkps_%d" % nb, _toy(P, [(1, (303.0, 200.0), [], [d0])], [(10, _at(P, 300.0, 200.0), [3], [d1])], {}, nb3dkps=nb),
                      [st], [kp]))
    # a stale observation under the snapshot rule: B is seen from keyframes 5 (alive) and 7 (gone); local point 11 is seen from 7.
    # Snapshot: 11 shares observer 7 with B.  (The reference removes 7 from B while it handles point 10, so it would match 11.)
    cases.append(("stale_observation_snapshot", _toy(P, [(1, (300.0, 200.0), [5, 7], [d0])],
                                                     [(10, _at(P, 300.5, 200.0), [3], [d1]), (11, _at(P, 300.25, 200.0), [7], [d0])],
                                                     {5: (_I7, {1: (300.0, 200.5)})}),
                  [BEST, NO_CANDIDATE], [0, -1]))
    # campt.z just below / at 0.1
    cases.append(("depth_threshold", _toy(P, [(1, (376.5, 240.0), [], [d0])],
                                          [(10, (0.0, 0.0, float(np.nextafter(0.1, 0))), [3], [d1]), (11, (0.0, 0.0, 0.1), [3], [d1])], {}),
                  [BEHIND, BEST], [-1, 0]))
    # the image's last column: x < img_w is strict, 752 itself is outside; 751.99 lies in the last cell column
    # (fy = 200: the vertical half-angle is the larger one, so the last column of the centre row is well inside the viewing cone)
    Pc = make_params(cam=dict(CRAFT_CAM, K=(400.0, 200.0, 376.0, 240.0)))
    cases.append(("last_column", _toy(Pc, [(1, (751.5, 240.0), [], [d0])],
                                      [(10, (0.94, 0.0, 1.0), [3], [d1]), (11, _at(Pc, 751.99, 240.0, 1.0), [3], [d1])], {}),
                  [OUT_OF_IMAGE, BEST], [-1, 0]))
    # more than 64 observers: the float sum runs over two chunks of lanes on the device, in ascending keyframe id
    n = 80
    kfs, ids = {}, list(range(100, 100 + 3 * n, 3))
    w = _at(P, 300.5, 200.0)
    for j, k in enumerate(ids):
        T = (0.01 * j, -0.005 * j, 0.0, 0.0, 0.0, 0.0, 1.0)
        px = project_dist(P, se3_act(pose(T), tuple(D(v) for v in w)))
        kfs[k] = (T, {1: (float(px[0]) + 0.37 + 0.01 * j, float(px[1]) - 0.21)})
    cases.append(("more_than_64_observers", _toy(P, [(1, (300.0, 200.0), ids, [d0, d1])], [(10, w, [3, 4], [d1, d0])], kfs),
                  [BEST], [0]))
    return cases
