"""ov2_btracker_track_mono (scope row f19) as the route of separate calls it replaces, on host mirrors of the frame pose, the motion
state and the keyframe info:
   1. motion.apply_batch on the mirrors
   2. LockstepTracker.trackFrameEpiPose with Twc and Tcw from step 1 (doepipolar False: trackFramePose)
   3. frame_after: the frame checkNewKfReq sees, built on the host by the rule of k_mono_pack -- the slots with (status & 3) == 1
      whose filter byte and pose byte are 0, none where the pose reset the frame; px is the tracked output, unpx / bv lastKeypoints
   4. motion.update_batch on the pose records' Twc
   5. keyframe.kf_decision_batch on those frames against the keyframes (kf_Tcw = keyframe.se3_inverse(kf_Twc))
The tracker's first frame: step 2 alone, from the mirrors' poses; the record is FIRST_FRAME.  The GPU test holds the fused step to
route() byte for byte."""
import numpy as np

from ov2slam_amd import _lib as L
from ov2slam_amd import keyframe, motion

_KF_INTS = ("n", "n_distinct", "n_nonfinite", "noccupcells", "nb3dkps", "n_out_of_grid", "decision", "reason")


def mirrors(batch):
    return dict(frames=0, poses=np.tile(np.array([0, 0, 0, 0, 0, 0, 1.0]), (batch, 1)), states=[motion.reset_state() for _ in range(batch)],
                keyframes=[None] * batch, info=[None] * batch)


def zero_decision(decision, reason):
    d = {k: 0 for k in _KF_INTS}
    d.update(parallax=np.float32(0), decision=decision, reason=reason)
    return d


def frame_after(st, n, epi, po):
    """the slots of the frame after the filter's and the pose's removals, ascending"""
    if po["action"] in (L.OV2_POSE_P3P_RESET, L.OV2_POSE_PNP_RESET):
        return np.zeros(0, np.int32)
    keep = (np.asarray(st)[:n] & 3) == 1
    if epi is not None:
        keep &= np.asarray(epi["removed"])[:n] == 0
    keep &= np.asarray(po["removed"])[:n] == 0
    return np.nonzero(keep)[0].astype(np.int32)


def route(ctx, trk, mir, imgs, kps, wpt, is3d, n, params, epi_params, p3p_req, seed, lmid, nbkfs, epi_seed, time, frame_id,
          localba_is_on=None, doepipolar=True, **kw):
    """-> (out, status, rule flags, epis or None, poses, monos); the mirrors are advanced"""
    na, B = len(imgs), trk.batch
    first = mir["frames"] == 0
    mir["frames"] += 1
    if first:
        states_a, Twc, rs = mir["states"][:na], mir["poses"][:na].copy(), np.zeros(na, np.uint8)
        Tcw = np.array([keyframe.se3_inverse(T) for T in Twc])
    else:
        states_a, Twc, Tcw, rs = motion.apply_batch(ctx, mir["states"][:na], mir["poses"][:na], np.asarray(time, np.float64)[:na])
    pad = lambda A: np.concatenate([A, np.tile(np.array([0, 0, 0, 0, 0, 0, 1.0]), (B - na, 1))])
    if doepipolar:
        out, st, rule, epis, poses = trk.trackFrameEpiPose(imgs, kps, wpt, is3d, pad(Tcw), n, params, epi_params, pad(Twc), p3p_req, seed, lmid,
                                                           nbkfs, epi_seed, **kw)
    else:
        out, st, rule, poses = trk.trackFramePose(imgs, kps, wpt, is3d, pad(Tcw), n, params, pad(Twc), p3p_req, seed, **kw)
        epis = None
    if first:
        monos = [dict(Twc_pred=Twc[b], resynced=0, state=mir["states"][b], kf=zero_decision(1, L.OV2_KF_FIRST_FRAME)) for b in range(na)]
        return out, st, rule, epis, poses, monos
    is3d = np.asarray(is3d, np.uint8).reshape(B, trk.n_max)
    lmid = np.asarray(lmid, np.int32).reshape(B, trk.n_max)
    items = []
    for b in range(na):
        nb = int(n[b])
        slots = frame_after(st[b], nb, None if epis is None else epis[b], poses[b])
        unpx, bv = trk.lastKeypoints(b, nb) if nb else (np.zeros((0, 2), np.float32), np.zeros((0, 3)))
        it = dict(cur_lmid=lmid[b, slots], cur_px=out[b, slots], cur_unpx=unpx[slots], cur_bv=bv[slots], cur_is3d=(is3d[b, slots] != 0),
                  cur_Twc=poses[b]["Twc"], cur_id=int(frame_id[b]), cur_time=float(time[b]),
                  localba_is_on=0 if localba_is_on is None else int(bool(localba_is_on[b])), noccupcells=-1, nb3dkps=-1)
        kf, info = mir["keyframes"][b], mir["info"][b]
        if kf is not None:
            it.update(kf_lmid=kf["lmid"], kf_unpx=kf["unpx"], kf_Tcw=keyframe.se3_inverse(kf["Twc"]))
        if info is not None:
            it.update(kf_id=info[0], kf_time=info[1], kf_nb3dkps=info[2])
        items.append(it)
    states_u = motion.update_batch(ctx, states_a, np.array([p["Twc"] for p in poses]), np.asarray(time, np.float64)[:na])
    decs = keyframe.kf_decision_batch(ctx, epi_params["fkf"], items)
    monos = []
    for b in range(na):
        kf = mir["keyframes"][b]
        if kf is None or len(kf["lmid"]) == 0 or mir["info"][b] is None:
            decs[b] = zero_decision(0, L.OV2_KF_NO_KEYFRAME)
        monos.append(dict(Twc_pred=Twc[b], resynced=int(rs[b]), state=states_u[b], kf=decs[b]))
        mir["poses"][b] = poses[b]["Twc"]
        mir["states"][b] = states_u[b]
    return out, st, rule, epis, poses, monos


def state_bytes(s):
    return np.concatenate([[s["prev_time"]], s["prevTwc"], s["log_relT"]]).astype(np.float64).tobytes()


def mono_bytes(m):
    """every field of a mono record, as bytes, field by field (so that a failing comparison names the field)"""
    d = dict(Twc_pred=np.asarray(m["Twc_pred"], np.float64).tobytes(), resynced=int(m["resynced"]), state=state_bytes(m["state"]),
             parallax=np.float32(m["kf"]["parallax"]).tobytes())
    d.update({k: int(m["kf"][k]) for k in _KF_INTS})
    return d
