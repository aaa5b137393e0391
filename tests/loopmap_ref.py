"""numpy restatement of the loop closer's local-map tracking (the reference's LoopCloser::trackLoopLocalMap and
LoopCloser::matchToMap, src/loop_closer.cpp:502-583 and :586-763) as include/ov2slam_hip.h specifies it for ov2_loop_match_to_map.
The pieces that are calls into other classes -- Frame::getSurroundingKeypoints, CameraCalibration::projectCamToImageDist,
Frame::isInImage, MapPoint::computeMinDescDist, the Sophus pose algebra -- are the ones of tests/match_ref.py and tests/tri_ref.py.

Two independent forms:
  replay()    the two reference functions statement by statement over a dict-based toy map: the covisible-keyframe walk that
              builds set_local_lmids and appends the (lmid, lmid) pairs, vmatchedkpids, the loop over the local set with its
              `continue`s, the pick, and the matches appended to vkplmids in std::map order;
  flat()      the per-local-map-point form over the flattened arrays of ov2_loopmap_item, i.e. what k_map_match<true>
              (csrc/mapmatch.hip) computes.
flatten() turns a toy map into those arrays (what the host does before the call); tests/test_loopmap_reference.py checks
replay == flat o flatten on every output field, bit for bit.  The loop only reads the map, so there is no deviation to document.

The iteration order of set_local_lmids (a std::unordered_set) is implementation-defined and decides the `<=` tie of the final pick:
replay() takes it as an explicit list, M["local_order"] (ids in the order the set would be iterated; ids it does not list follow
in insertion order).  ov2slam_amd/host/loop_closer.hpp reproduces the real order with a literal std::unordered_set.

Arithmetic: np.float64 where the reference holds a double, np.float32 (`# f32`) where it holds a float.  view_th =
cos(atan(hfov)) is taken in double and rounded to float per step."""
import copy
import math

import numpy as np

from tests import match_ref as MR
from tests.match_ref import (BEHIND, BEST, EUROC, FISHEYE4, NO_CANDIDATE, OUT_OF_FOV, OUT_OF_IMAGE, RADTAN4, RADTAN5, RATIO_REJECTED,
                             _min_desc_dist, grid_width, hamming, in_image, project_dist, same)
from tests.tri_ref import D, F32, norm3, pose, pt_dist, se3_act

WINDOW = 15                                                             # kfid < lckf.kfid_ - 15 / > lckf.kfid_ + 15
FDISTRATIO = float(F32(0.2 * 1.5))                                      # (float)(fmax_desc_dist_ * 1.5), fmax_desc_dist_ = 0.2


def make_params(D=None, model="pinhole", cam=EUROC, fmax_proj_pxdist=10.0, fmax_desc_dist=FDISTRATIO):
    """the settings LoopCloser::processLoopCandidate passes: maxdist 10., ratio fmax_desc_dist_ * 1.5"""
    return dict(model=model, K=tuple(cam["K"]), D=None if D is None else tuple(D), img_w=cam["img_w"], img_h=cam["img_h"],
                ncellsize=cam["ncellsize"], fmax_proj_pxdist=fmax_proj_pxdist, fmax_desc_dist=fmax_desc_dist)


def thresholds(P):
    """:595-607 and :656: (view_th, dmaxpxdist, mindist), floats.  hfov is the half width TIMES fx, and atan(hfov) is taken in
    both branches of the reference's `if`, so vfov never matters."""
    fx = D(P["K"][0])
    hfov = F32(D(0.5) * D(P["img_w"]) * fx)                             # f32
    maxradfov = F32(math.atan(float(hfov)))                             # f32
    view_th = F32(math.cos(float(maxradfov)))                           # f32
    dmax = F32(P["fmax_proj_pxdist"])
    mindist = F32(D(F32(P.get("desc_bytes", 32)) * F32(P["fmax_desc_dist"])) * D(8))   # int * float, * 8., stored to float
    return view_th, dmax, mindist


def _ev(ev, key, n=1):
    if ev is not None:
        ev[key] = ev.get(key, 0) + n


def _margin(ev, *vals):
    MR._margin(ev, *vals)


def _iteration(members, order):
    """the members of the set in the order M["local_order"] dictates (module docstring)"""
    rank = {i: r for r, i in enumerate(order or [])}
    listed = sorted((i for i in members if i in rank), key=rank.get)
    return listed + [i for i in members if i not in rank]


# ---- (a) the reference, literally, over the toy map ----------------------------------------------------------------------------------
def replay(M, ev=None):
    """LoopCloser::trackLoopLocalMap(newkf, lckf, Twc, maxdist, ratio, vkplmids).  M: params, newkf (kfid_, mapkps_ {lmid: px_},
    vgridkps_ [cell][...] of keypoint ids), Tcw (7: Twc.inverse()), lckf (kfid_, cov {kfid: score}: getCovisibleKfMap()), cokfs
    {kfid: [lmid ...]} (the keyframes the map holds, with the lmid_ of getKeypoints3d() in order), mps {lmid: is3d_, bad, wpt,
    set_kfids_, map_kf_desc_ {kfid: 32 bytes}}, vkplmids [(kpid, lmid) ...] as the earlier stages left it, local_order.
    Returns (vkplmids, info) with info: walk_vkplmids (the list after the walk), local (set_local_lmids in iteration order),
    map_previd_newid, kp_dist, diag[lmid] = (status, bestid, bestdist, projpx) for every local id past the host-side filters."""
    newkf, lckf = M["newkf"], M["lckf"]
    vkplmids = list(M["vkplmids"])
    set_local_lmids, set_checked_kpids = [], set()                      # a list for the insertion order, used as a set
    lccov_map = dict(lckf["cov"])
    lccov_map[lckf["kfid_"]] = 100
    for kfid in sorted(lccov_map):                                      # std::map: ascending keyframe id
        if kfid < lckf["kfid_"] - WINDOW:
            _ev(ev, "walk_below")
            continue
        elif kfid > lckf["kfid_"] + WINDOW:
            _ev(ev, "walk_above")
            break
        pcokf = M["cokfs"].get(kfid)
        if pcokf is None:
            _ev(ev, "walk_missing")
            continue
        for lmid in pcokf:
            if lmid not in set_checked_kpids:
                set_checked_kpids.add(lmid)
                if lmid in newkf["mapkps_"]:                            # newkf.isObservingKp(kp.lmid_)
                    kplmid = (lmid, lmid)
                    if kplmid not in vkplmids:
                        vkplmids.append(kplmid)
                elif lmid not in set_local_lmids:
                    set_local_lmids.append(lmid)
    vmatchedkpids = []
    for kpid, lmid in vkplmids:
        vmatchedkpids.append(kpid)
        if lmid in set_local_lmids:
            set_local_lmids.remove(lmid)
            _ev(ev, "walk_erased")
    info = dict(walk_vkplmids=list(vkplmids), local=_iteration(set_local_lmids, M.get("local_order")))
    map_previd_newid = _replay_match(M, vmatchedkpids, info["local"], info, ev)
    for kpid in sorted(map_previd_newid):                               # std::map iteration
        vkplmids.append((kpid, map_previd_newid[kpid]))
    return vkplmids, info


def _replay_match(M, vmatchedkpids, local, info, ev):
    """LoopCloser::matchToMap(frame, Tcw, fmaxprojerr, fdistratio, vmatchedkpids, set_local_lmids)"""
    P, frame, mps = M["params"], M["newkf"], M["mps"]
    map_previd_newid, diag = {}, {}
    info.update(map_previd_newid=map_previd_newid, diag=diag, kp_dist={})
    if not local:
        return map_previd_newid
    view_th, dmaxpxdist, _ = thresholds(P)
    nbwcells = grid_width(P)[0]
    Tcw = pose(M["Tcw"])
    map_kpids_vlmidsdist = {}
    for lmid in local:
        if lmid in frame["mapkps_"]:                                    # frame.isObservingKp(lmid)
            continue
        plm = mps.get(lmid)
        if plm is None:
            continue
        elif not plm["is3d_"] or plm.get("bad", False):
            continue
        wpt = tuple(D(v) for v in plm["wpt"])
        if not plm["map_kf_desc_"]:                                     # lmdesc.empty()
            continue
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
        mindist = thresholds(P)[2]
        bestid, secid = -1, -1
        bestdist, secdist = mindist, mindist
        for kp_lmid, kp_px in vnearkps:
            if kp_lmid in vmatchedkpids:
                _ev(ev, "gate_matched")
                continue
            if kp_lmid < 0:
                continue
            pxdist = F32(pt_dist(projpx, kp_px))                        # f32
            _margin(ev, D(pxdist) - D(dmaxpxdist))
            if pxdist > dmaxpxdist:
                _ev(ev, "gate_pxdist")
                continue
            pkplm = mps.get(kp_lmid)
            if pkplm is None:
                _ev(ev, "gate_nomp")
                continue
            elif not pkplm["map_kf_desc_"]:
                _ev(ev, "gate_nomp")
                continue
            is_candidate = True
            set_plmkfs = set(plm["set_kfids_"])
            for kfid in pkplm["set_kfids_"]:
                if kfid in set_plmkfs:
                    is_candidate = False
                    break
            if not is_candidate:
                _ev(ev, "gate_shared")
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
    for kpid in sorted(map_kpids_vlmidsdist):
        bestdist, bestlmid = F32(1024), -1
        for lmid, d in map_kpids_vlmidsdist[kpid]:
            if d <= bestdist:
                if bestlmid >= 0 and d == bestdist:
                    _ev(ev, "tie_pick")
                bestdist, bestlmid = d, lmid
        if bestlmid >= 0:
            map_previd_newid[kpid] = bestlmid
            info["kp_dist"][kpid] = bestdist
    return map_previd_newid


# ---- the host's flattening -------------------------------------------------------------------------------------------------------------
def local_set(M):
    """the set-building walk :505-562 in set algebra: (vkplmids after the walk, set_local_lmids in iteration order)"""
    lc = M["lckf"]["kfid_"]
    ids = []
    for kfid in sorted(set(M["lckf"]["cov"]) | {lc}):
        if lc - WINDOW <= kfid <= lc + WINDOW and kfid in M["cokfs"]:
            ids += [i for i in M["cokfs"][kfid]]
    ids = list(dict.fromkeys(ids))                                      # first occurrence, in walk order
    observed = M["newkf"]["mapkps_"]
    vk = list(M["vkplmids"])
    have = set(vk)
    for i in ids:
        if i in observed and (i, i) not in have:
            vk.append((i, i)); have.add((i, i))
    paired = {l for _, l in vk}
    return vk, _iteration([i for i in ids if i not in observed and i not in paired], M.get("local_order"))


def flatten(M):
    """(item, meta): the arrays of ov2_loopmap_item for the toy map, and meta = dict(kp_lmid, lm_lmid, walk_vkplmids) to map rows
    back to ids.  Map-point rows: ascending lmid; keypoint rows: the order of newkf.mapkps_."""
    P, frame, mps = M["params"], M["newkf"], M["mps"]
    vk, local = local_set(M)
    matched = {k for k, _ in vk}
    kp_lmid = list(frame["mapkps_"].keys())
    lm_lmid = [i for i in local if i not in frame["mapkps_"] and i in mps and mps[i]["is3d_"] and not mps[i].get("bad", False) and
               mps[i]["map_kf_desc_"]]
    rows = sorted(set(lm_lmid) | {i for i in kp_lmid if i in mps and mps[i]["map_kf_desc_"]})
    row_of = {i: r for r, i in enumerate(rows)}
    obs_start, obs_kfid, desc_start, desc = [0], [], [0], []
    for i in rows:
        obs_kfid.extend(sorted(mps[i]["set_kfids_"]))
        obs_start.append(len(obs_kfid))
        desc.extend(mps[i]["map_kf_desc_"].values())
        desc_start.append(len(desc))
    kp_row = {i: r for r, i in enumerate(kp_lmid)}
    cell_start, cell_kp = [0], []
    nbw, nbh = grid_width(P)
    for c in range(nbw * nbh):
        cell_kp.extend(kp_row[i] for i in frame["vgridkps_"][c] if i in kp_row)
        cell_start.append(len(cell_kp))
    item = dict(Tcw=np.asarray(M["Tcw"], np.float64),
                kp_px=np.asarray([frame["mapkps_"][i] for i in kp_lmid], np.float32).reshape(-1, 2),
                kp_mp=np.asarray([row_of.get(i, -1) if i >= 0 else -1 for i in kp_lmid], np.int32),
                kp_matched=np.asarray([1 if i in matched else 0 for i in kp_lmid], np.uint8),
                cell_start=np.asarray(cell_start, np.int32), cell_kp=np.asarray(cell_kp, np.int32),
                obs_start=np.asarray(obs_start, np.int32), obs_kfid=np.asarray(obs_kfid, np.int32),
                desc_start=np.asarray(desc_start, np.int32), desc=np.asarray(desc, np.uint8).reshape(-1, 32),
                lm_mp=np.asarray([row_of[i] for i in lm_lmid], np.int32),
                lm_wpt=np.asarray([mps[i]["wpt"] for i in lm_lmid], np.float64).reshape(-1, 3))
    return item, dict(kp_lmid=kp_lmid, lm_lmid=lm_lmid, walk_vkplmids=vk)


def _empty(n_lm, n_kp):
    return MR._empty(n_lm, n_kp)


def replay_arrays(M, meta, ev=None):
    """replay() in the layout of flat()'s result, plus the final vkplmids"""
    vk, info = replay(copy.deepcopy(M), ev=ev)
    kp_row = {i: r for r, i in enumerate(meta["kp_lmid"])}
    lm_row = {i: r for r, i in enumerate(meta["lm_lmid"])}
    assert sorted(info["diag"]) == sorted(meta["lm_lmid"]), "the host-side filters of flatten() and replay() disagree"
    out = _empty(len(meta["lm_lmid"]), len(meta["kp_lmid"]))
    for l, lmid in enumerate(meta["lm_lmid"]):
        st, bestid, bestdist, px = info["diag"][lmid]
        out["lm_status"][l] = st
        out["lm_kp"][l] = kp_row[bestid] if st == BEST else -1
        out["lm_dist"][l] = bestdist
        out["lm_projpx"][l] = px
    for kpid, lmid in info["map_previd_newid"].items():
        out["kp_lm"][kp_row[kpid]] = lm_row[lmid]
        out["kp_dist"][kp_row[kpid]] = info["kp_dist"][kpid]
    out["n_matches"] = len(info["map_previd_newid"])
    return out, vk


def vkplmids_of(out, meta):
    """what trackLoopLocalMap leaves in vkplmids, from a flat / device result: the walk's list, then (kp_lmid, lm_lmid) of the
    matches in ascending keypoint id (:576-582)"""
    new = sorted((meta["kp_lmid"][k], meta["lm_lmid"][int(l)]) for k, l in enumerate(out["kp_lm"]) if l >= 0)
    return list(meta["walk_vkplmids"]) + new


# ---- (b) the per-local-map-point form over the flattened arrays ----------------------------------------------------------------------
def flat(P, item, ev=None):
    """what ov2_loop_match_to_map returns for (params, item): a dict of the arrays of ov2_loopmap_result"""
    view_th, dmax, mindist = thresholds(P)
    nbw = grid_width(P)[0]
    cs = F32(P["ncellsize"])
    T = pose(item["Tcw"])
    obs_start, desc_start, cell_start = item["obs_start"], item["desc_start"], item["cell_start"]
    n_lm, n_kp = len(item["lm_mp"]), len(item["kp_mp"])
    out = _empty(n_lm, n_kp)
    proposals = [[] for _ in range(n_kp)]
    for l in range(n_lm):
        w = tuple(D(v) for v in item["lm_wpt"][l])
        A = int(item["lm_mp"][l])
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
        idsA = set(int(v) for v in item["obs_kfid"][obs_start[A]:obs_start[A + 1]])
        descA = item["desc"][desc_start[A]:desc_start[A + 1]]
        bestid, secid, bestdist, secdist = -1, -1, mindist, mindist
        nsurv = 0
        for r in (rkp - 1, rkp):
            for c in (ckp - 1, ckp):
                if r < 0 or c < 0:
                    continue
                idx = r * nbw + c
                for k in item["cell_kp"][cell_start[idx]:cell_start[idx + 1]]:
                    k = int(k)
                    _ev(ev, "block_kp")
                    if item["kp_matched"][k]:
                        _ev(ev, "gate_matched")
                        continue
                    B = int(item["kp_mp"][k])
                    if B < 0:
                        _ev(ev, "gate_nomp")
                        continue
                    descB = item["desc"][desc_start[B]:desc_start[B + 1]]
                    if len(descB) == 0:
                        _ev(ev, "gate_nomp")
                        continue
                    pxdist = F32(pt_dist(px, item["kp_px"][k]))         # f32
                    _margin(ev, D(pxdist) - D(dmax))
                    if pxdist > dmax:
                        _ev(ev, "gate_pxdist")
                        continue
                    nsurv += 1
                    o0, o1 = int(obs_start[B]), int(obs_start[B + 1])
                    if any(int(v) in idsA for v in item["obs_kfid"][o0:o1]):
                        _ev(ev, "gate_shared")
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
        _ev(ev, "in_image")
        _ev(ev, "survivors", nsurv)
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


def matched_flag_effects(P, item):
    """(takeovers, unrejected): local points whose proposal the matched flags change in the two ways the header names -- without
    the flags the point's best keypoint is a flagged one and with them another keypoint takes over; without the flags the point
    is RATIO_REJECTED and with them BEST.  From flat() alone."""
    with_flags = flat(P, item)
    clear = dict(item); clear["kp_matched"] = np.zeros_like(item["kp_matched"])
    without = flat(P, clear)
    flagged = item["kp_matched"].astype(bool)
    w_kp, o_kp = with_flags["lm_kp"], without["lm_kp"]
    take = (without["lm_status"] == BEST) & (with_flags["lm_status"] == BEST) & (o_kp >= 0) & flagged[np.maximum(o_kp, 0)] & (w_kp != o_kp)
    unrej = (without["lm_status"] == RATIO_REJECTED) & (with_flags["lm_status"] == BEST)
    return np.nonzero(take)[0], np.nonzero(unrej)[0]


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------
def make_scene(P, rng, *, n_kp=120, n_lm=261, n_kf=8, matched=1 / 3, many_obs=0, max_obs=4, dup=0.6, fov_points=3):
    """A toy loop candidate.  The new keyframe, its keypoints with their map points and the planted local points (duplicates,
    ratio-test twins, descriptor ties, competing proposals, shared observers, points all around the camera) come from
    match_ref.make_scene; on top of it: the loop keyframe's covisibility map with keyframes below, inside and above the +-15
    window and one the map no longer holds, the local points spread over those keyframes' 3-D keypoints (some twice, some only
    in keyframes outside the window), keypoints of the new keyframe among them (the (lmid, lmid) pairs), a vkplmids that flags
    about `matched` of the keypoints (half of them paired with their planted duplicate, which then leaves the local set), bad
    map points, and fov_points points below the (tiny) viewing-cone threshold."""
    M0 = MR.make_scene(P, rng, n_kp=n_kp, n_lm=n_lm, n_kf=n_kf, many_obs=many_obs, max_obs=max_obs, dup=dup)
    frame, mps = M0["frame"], M0["mps"]
    Tcw = frame["Tcw"]
    local = list(M0["local"])
    next_id = max(list(mps) + [2000]) + 1
    for _ in range(fov_points):                                         # z / |p| below 5.8e-6: only a point next to the image plane, kilometres away
        z = rng.uniform(0.1, 0.14)
        ang = rng.uniform(0, 2 * np.pi)
        pc = np.array([3e4 * np.cos(ang), 3e4 * np.sin(ang), z])
        mps[next_id] = dict(is3d_=True, wpt=MR._inv_act(Tcw, pc), set_kfids_=[3], map_kf_desc_={3: rng.integers(0, 256, 32).astype(np.uint8)})
        local.insert(int(rng.integers(0, len(local) + 1)), next_id)
        next_id += 1
    for lmid in local:                                                  # isBad()
        if lmid in mps and rng.uniform() < 0.03:
            mps[lmid]["bad"] = True
    lc = 200
    inside = sorted(int(v) for v in rng.choice(np.arange(lc - WINDOW, lc + WINDOW + 1), size=5, replace=False))
    if lc + WINDOW not in inside and rng.uniform() < 0.5:
        inside.append(lc + WINDOW)
    if lc - WINDOW not in inside and rng.uniform() < 0.5:
        inside.append(lc - WINDOW)
    inside = sorted(set(inside) | {lc})
    outside = [lc - WINDOW - 1 - int(rng.integers(0, 9)), lc - WINDOW - 1, lc + WINDOW + 1, lc + WINDOW + 2 + int(rng.integers(0, 9))]
    gone = [k for k in range(lc - WINDOW, lc + WINDOW + 1) if k not in inside][int(rng.integers(0, 5))]
    cov = {k: int(rng.integers(1, 60)) for k in inside + outside + [gone]}
    if rng.uniform() < 0.5:
        cov.pop(lc)                                                     # the loop keyframe is not in its own covisibility map: added with score 100
    cokfs = {k: [] for k in inside + outside}
    observed = list(frame["mapkps_"])
    for lmid in local + [int(v) for v in rng.choice(observed, size=min(len(observed), 12), replace=False)]:
        u = rng.uniform()
        homes = [int(v) for v in rng.choice(inside, size=2 if u < 0.3 else 1, replace=False)] if u < 0.95 else [int(rng.choice(outside))]
        for k in homes:
            cokfs[k].append(lmid)
            if rng.uniform() < 0.05:
                cokfs[k].append(lmid)                                   # listed twice in one keyframe: set_checked_kpids
    for k in cokfs:
        cokfs[k] = [cokfs[k][i] for i in rng.permutation(len(cokfs[k]))]
    dup_of = {b: a for a, b in M0["planted"]}
    vk = []
    for kpid in observed:
        if rng.uniform() < matched:
            if kpid in dup_of and rng.uniform() < 0.5:
                vk.append((kpid, dup_of[kpid]))
            elif rng.uniform() < 0.15:
                vk.append((kpid, kpid))                                 # already paired with itself: no second (lmid, lmid) pair
            else:
                vk.append((kpid, 500000 + int(rng.integers(0, 1000))))
    everyone = sorted({i for ids in cokfs.values() for i in ids})
    local_order = [everyone[i] for i in rng.permutation(len(everyone))]
    return dict(params=P, newkf=dict(kfid_=frame["kfid_"], mapkps_=frame["mapkps_"], vgridkps_=frame["vgridkps_"]), Tcw=np.asarray(Tcw),
                lckf=dict(kfid_=lc, cov=cov), cokfs=cokfs, mps=mps, vkplmids=vk, local_order=local_order, planted=M0["planted"])


def filtered_scene(P, seed, min_margin=1e-3, **kw):
    """make_scene, resampled until no gate quantity of the flat form lies within min_margin px of its threshold"""
    for t in range(200):
        M = make_scene(P, np.random.default_rng(1000 * seed + t), **kw)
        item, meta = flatten(M)
        ev = {}
        ref = flat(P, item, ev)
        if ev.get("margin", np.inf) >= min_margin:
            return M, item, meta, ref
    raise RuntimeError("no scene with the requested margin")


def trim(item, meta, n_lm):
    """the item with its first n_lm local map points only (the map-point table stays)"""
    it = dict(item); it["lm_mp"] = item["lm_mp"][:n_lm]; it["lm_wpt"] = item["lm_wpt"][:n_lm]
    return it, dict(meta, lm_lmid=meta["lm_lmid"][:n_lm])


# ---- crafted cases ---------------------------------------------------------------------------------------------------------------------------
CRAFT_CAM = MR.CRAFT_CAM
_I7 = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)


def toy(P, kps, local, vkplmids=(), lc=50):
    """kps: [(lmid, px, kfids, descs) or (lmid, px, None)] (None: the keypoint's map point is gone); local: [(lmid, wpt, kfids,
    descs)], all 3-D keypoints of the loop keyframe in that order (which is also the iteration order).  The pose is the identity:
    camera frame = world frame."""
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
    ids = [l[0] for l in local]
    return dict(params=P, newkf=dict(kfid_=77, mapkps_=mapkps, vgridkps_=vgrid), Tcw=np.asarray(_I7), lckf=dict(kfid_=lc, cov={}),
                cokfs={lc: ids}, mps=mps, vkplmids=list(vkplmids), local_order=ids, planted=[])


def _at(P, u, v, z=4.0):
    return MR._at(P, u, v, z)


def _desc(seed, n=1):
    return [np.random.default_rng(seed * 100 + i).integers(0, 256, 32).astype(np.uint8) for i in range(n)]


def _flip(d, bits):
    d = np.array(d, np.uint8)
    for b in bits:
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def crafted_cases():
    """[(name, M, expected lm_status list, expected lm_kp list)]; identity pose, no distortion: a point built with _at() projects
    onto the pixel it names (to float rounding)"""
    P = make_params(cam=CRAFT_CAM)
    d0 = np.arange(32, dtype=np.uint8)
    cases = []
    # 70 keypoints in the 2x2 block, all within 10 px: two chunks of lanes; the 67th is the only exact copy
    kps = [(100 + i, (300.0 + 0.1 * (i % 10), 200.0 + 0.1 * (i // 10)), [5], [_flip(d0, range(3, 3 + 20 + (i % 7)))]) for i in range(70)]
    kps[66] = (166, kps[66][1], [5], [d0.copy()])
    cases.append(("block_of_70_keypoints", toy(P, kps, [(10, _at(P, 300.5, 200.5), [3], [d0])]), [BEST], [66]))
    # a candidate with 80 observations, none shared / the 80th shared
    ids80 = list(range(100, 100 + 3 * 80, 3))
    cases.append(("candidate_with_80_observations", toy(P, [(1, (300.0, 200.0), ids80, [d0])],
                                                        [(10, _at(P, 300.5, 200.0), [3, 101, 400], [_flip(d0, [1])]),
                                                         (11, _at(P, 301.0, 200.0), [3, ids80[79]], [_flip(d0, [2])])]),
                  [BEST, NO_CANDIDATE], [0, -1]))
    # 9 x 9 = 81 descriptor pairs, the only close pair is the last one (pair 80, second chunk); and 1 x 1
    A9 = _desc(1, 8) + [d0.copy()]
    B9 = _desc(2, 8) + [_flip(d0, [7])]
    cases.append(("81_and_1_descriptor_pairs", toy(P, [(1, (300.0, 200.0), [5], B9), (2, (500.0, 300.0), [5], [d0])],
                                                   [(10, _at(P, 300.5, 200.0), [3], A9), (11, _at(P, 500.5, 300.0), [3], [_flip(d0, [9, 10])])]),
                  [BEST, BEST], [0, 1]))
    # projections in cell row 0 / column 0 (r - 1, c - 1 skipped, not wrapped) and in the last cell
    Pw = make_params(cam=dict(CRAFT_CAM, K=(400.0, 200.0, 376.0, 240.0)))
    cases.append(("first_row_first_column_last_cell",
                  toy(Pw, [(1, (5.0, 5.0), [5], [d0]), (2, (748.0, 476.0), [5], [_flip(d0, [4])]), (3, (745.0, 30.0), [5], [d0])],
                      [(10, _at(Pw, 6.0, 6.0, 1.0), [3], [_flip(d0, [1])]), (11, _at(Pw, 750.0, 478.0, 1.0), [3], [_flip(d0, [2])]),
                       (12, _at(Pw, 3.0, 40.0, 1.0), [3], [_flip(d0, [3])])]),
                  [BEST, BEST, NO_CANDIDATE], [0, 1, -1]))
    # c = -1 is skipped, not wrapped into the previous row's last cell: with a 2000 px radius the keypoint there would match
    Pr = make_params(cam=dict(CRAFT_CAM, K=(400.0, 200.0, 376.0, 240.0)), fmax_proj_pxdist=2000.0)
    cases.append(("column_minus_one_skipped", toy(Pr, [(1, (745.0, 50.0), [5], [d0])], [(10, _at(Pr, 10.0, 100.0, 1.0), [3], [_flip(d0, [1])])]),
                  [NO_CANDIDATE], [-1]))
    # equal-distance proposals to one keypoint: the point listed later wins; a closer one listed earlier wins over both
    cases.append(("equal_proposals_later_wins", toy(P, [(1, (300.0, 200.0), [5], [d0]), (2, (500.0, 300.0), [5], [d0])],
                                                    [(10, _at(P, 300.5, 200.0), [3], [_flip(d0, [1])]), (11, _at(P, 299.5, 200.0), [3], [_flip(d0, [2])]),
                                                     (12, _at(P, 500.5, 300.0), [3], [d0]), (13, _at(P, 499.5, 300.0), [3], [_flip(d0, [2])])]),
                  [BEST, BEST, BEST, BEST], [0, 0, 1, 1]))
    # a `<=` tie among candidates: the later keypoint becomes best, the earlier second; 0.9 * 0 < 0 is false, so BEST
    cases.append(("tie_among_candidates", toy(P, [(1, (300.0, 200.0), [5], [d0]), (2, (301.0, 200.0), [5], [d0])],
                                              [(10, _at(P, 300.5, 200.0), [3], [d0])]),
                  [BEST], [1]))
    # matched flag, first effect: keypoint 1 would be best (distance 0) but is in vmatchedkpids: keypoint 2 (distance 3) takes over
    cases.append(("matched_best_excluded_second_takes_over",
                  toy(P, [(1, (300.0, 200.0), [5], [d0]), (2, (301.0, 200.0), [5], [_flip(d0, [1, 2, 3])])],
                      [(10, _at(P, 300.5, 200.0), [3], [d0])], vkplmids=[(1, 4711)]),
                  [BEST], [1]))
    # second effect: two keypoints at distances 20 and 21 trip the ratio test; with the second one flagged the point is BEST
    t20, t21 = _flip(d0, range(20)), _flip(d0, range(100, 121))
    for name, vk, st, kp in (("ratio_rejected_without_flag", [], RATIO_REJECTED, -1), ("matched_exclusion_unrejects", [(2, 4711)], BEST, 0)):
        cases.append((name, toy(P, [(1, (300.0, 200.0), [5], [t20]), (2, (301.0, 200.0), [5], [t21])],
                                [(10, _at(P, 300.5, 200.0), [3], [d0])], vkplmids=vk), [st], [kp]))
    # the viewing cone: only a point next to the image plane and kilometres to the side falls below cos(atan(0.5 img_w fx));
    # 1e3 to the side passes the cone and leaves the image
    cases.append(("out_of_fov_and_out_of_image", toy(make_params(), [(1, (300.0, 200.0), [5], [d0])],
                                                     [(10, (2.5e4, 0.0, 0.1), [3], [d0]), (11, (1e3, 0.0, 0.1), [3], [d0])]),
                  [OUT_OF_FOV, OUT_OF_IMAGE], [-1, -1]))
    # a keypoint whose map point is gone, and the shared-observer gate
    cases.append(("gone_map_point_and_shared_observer",
                  toy(P, [(1, (300.0, 200.0), None), (2, (301.0, 200.0), [3, 9], [d0])], [(10, _at(P, 300.5, 200.0), [9], [d0])]),
                  [NO_CANDIDATE], [-1]))
    cases.append(("one_local_point", toy(P, [(1, (300.0, 200.0), [5], [d0])], [(10, _at(P, 300.5, 200.0), [3], [_flip(d0, [1])])]), [BEST], [0]))
    cases.append(("no_keypoint", toy(P, [], [(10, _at(P, 300.5, 200.0), [3], [d0])]), [NO_CANDIDATE], [-1]))
    cases.append(("no_local_point", toy(P, [(1, (300.0, 200.0), [5], [d0])], []), [], []))
    return cases
