"""The lock-step step with epipolar2d2dFiltering and the pose fused in (ov2_btracker_track_frame_epi_pose, scope row f18) as the route
of separate calls it replaces, built from what exists:
   frame_set      which slots of an item are the frame after kltTracking removed the lost keypoints, in which order
   route          trackFrameMap -> frame_set on the host -> keyframe.epipolar_filter_batch (kf_Tcw = keyframe.se3_inverse(kf_Twc), as
                  LockstepTracker.setKeyframe derives it) -> the removals taken out of framepose_ref.pose_set -> ov2_p3p_draw_samples
                  -> pose.compute_pose_batch -> both `removed` arrays, err and pair_cur scattered back to slot space
The GPU test holds the fused step to route() byte for byte."""
import numpy as np

from ov2slam_amd import keyframe, pose
from tests import framepose_ref as F

_SCALARS = ("action", "m", "epifrom3dkps", "do_optimize", "nb3dkps", "status", "best_row", "iterations", "rows_consumed", "n_inliers",
            "n_outliers", "n_removed_ransac", "n_removed_sampson", "pose_from_model")


def frame_set(status, n):
    """the slots i < n with (status[i] & 3) == 1, ascending"""
    return np.nonzero((np.asarray(status)[:n] & 3) == 1)[0].astype(np.int32)


def nothing_ran(n):
    """the epipolar record of an item on a tracker's first frame and on a step where nothing is tracked"""
    d = {k: 0 for k in _SCALARS}
    d.update(action=keyframe.EPIF_TOO_FEW_KPS, parallax=np.float32(0), score=np.float64(0), model=np.zeros(12), F=np.zeros(9),
             Twc_model=np.zeros(7), removed=np.zeros(n, np.uint8), err=np.zeros(n, np.float32), pair_cur=np.zeros(0, np.int32))
    return d


def route(ctx, trk, imgs, kps, wpt, is3d, Tcw, n, params, epi_params, Twc, p3p_req, seed, lmid, nbkfs, epi_seed, keyframes, scale=None,
          dop3p=False, n_rows=0, klt_use_prior=True):
    """keyframes[b]: None or dict(lmid, unpx, bv, Twc).  -> (out, status, p3p flags of the rule, epis, poses, epi_inputs,
    pose_inputs): epis[b] as keyframe.epipolar_filter returns it with removed / err (n[b],) and pair_cur (m,) in slot space; poses[b]
    as framepose_ref.route; epi_inputs[b] = (n_cur, slots, m, samples (rows used, 8)); pose_inputs[b] = (m, slots, samples)"""
    out, st, rule = trk.trackFrameMap(imgs, kps, wpt, is3d, Tcw, n, klt_use_prior=klt_use_prior)
    na = len(imgs)
    wpt = np.asarray(wpt, np.float64).reshape(trk.batch, trk.n_max, 3)
    is3d = np.asarray(is3d, np.uint8).reshape(trk.batch, trk.n_max)
    lmid = np.asarray(lmid, np.int32).reshape(trk.batch, trk.n_max)
    Twc = np.asarray(Twc, np.float64).reshape(-1, 7)
    rows = int(epi_params["n_rows"])
    items, frames, kp = [], [], []
    for b in range(na):
        nb = int(n[b])
        slots = frame_set(st[b], nb)
        unpx, bv = trk.lastKeypoints(b, nb) if nb else (np.zeros((0, 2), np.float32), np.zeros((0, 3)))
        it = dict(cur_lmid=lmid[b, slots], cur_px=out[b, slots], cur_unpx=unpx[slots], cur_bv=bv[slots], cur_is3d=is3d[b, slots],
                  cur_Twc=Twc[b], nb3dkps=-1, nbkfs=int(nbkfs[b]), seed=int(epi_seed[b]))
        kf = keyframes[b]
        if kf is not None:
            it.update(kf_lmid=kf["lmid"], kf_unpx=kf["unpx"], kf_bv=kf["bv"], kf_Twc=kf["Twc"], kf_Tcw=keyframe.se3_inverse(kf["Twc"]))
        items.append(it); frames.append(slots); kp.append((unpx, bv))
    epis = keyframe.epipolar_filter_batch(ctx, epi_params, items, trace_samples=True)
    epi_inputs, problems, pose_inputs = [], [], []
    for b in range(na):
        nb, slots, e = int(n[b]), frames[b], epis[b]
        rm, er = np.zeros(nb, np.uint8), np.zeros(nb, np.float32)
        rm[slots], er[slots] = e["removed"], e["err"]
        tab = e.pop("samples")
        epi_inputs.append((len(slots), slots, e["m"], np.zeros((0, 8), np.int32) if tab is None or rows == 0 else tab))
        e.update(removed=rm, err=er, pair_cur=slots[e["pair_cur"]])
        # the frame after the filter, then exactly framepose_ref.route
        sel = F.pose_set(np.where(rm != 0, 0, st[b, :nb]), is3d[b], nb)
        m = len(sel)
        unpx, bv = kp[b]
        req = bool(p3p_req[b]) or bool(rule[b])
        do_p3p = req or bool(dop3p)
        ptab = pose.draw_samples(int(seed[b]), m, n_rows) if do_p3p and m >= 4 else np.zeros((0, 4), np.int32)
        sc = np.zeros(m, np.int32) if scale is None else np.asarray(scale, np.int32).reshape(trk.batch, trk.n_max)[b, sel]
        problems.append(dict(unpx=unpx[sel].astype(np.float64), wpt=wpt[b, sel], scale=sc, Twc=Twc[b], bv=bv[sel], do_p3p=do_p3p,
                             p3p_req=req, samples=ptab))
        pose_inputs.append((m, sel, ptab))
    poses = pose.compute_pose_batch(ctx, params, problems)
    for b in range(na):
        rm = np.zeros(int(n[b]), np.uint8)
        rm[pose_inputs[b][1]] = poses[b]["removed"]
        poses[b]["removed"] = rm
    return out, st, rule, epis, poses, epi_inputs, pose_inputs


def epi_bytes(e):
    """every field of an epipolar record, as bytes, field by field (so that a failing comparison names the field)"""
    d = {k: int(e[k]) for k in _SCALARS}
    d.update(parallax=np.float32(e["parallax"]).tobytes(), score=np.float64(e["score"]).tobytes(),
             model=np.asarray(e["model"], np.float64).tobytes(), F=np.asarray(e["F"], np.float64).tobytes(),
             Twc_model=np.asarray(e["Twc_model"], np.float64).tobytes(), removed=np.asarray(e["removed"], np.uint8).tobytes(),
             err=np.asarray(e["err"], np.float32).tobytes(), pair_cur=np.asarray(e["pair_cur"], np.int32).tobytes())
    return d
