"""ov2_btracker_create_keyframe (scope row f20) as the route of separate calls it replaces, on the existing Python calls:
   1. LockstepTracker.describeBRIEF of the frame's keypoints (use_brief)
   2. tests/kfreq_ref.py: replay_counts -> noccupcells, nb3dkps; nb2detect = nbmaxkps - noccupcells
   3. LockstepTracker.detectSingleScale / detectGridFAST over the batch with the frames' keypoints as the occupied set; the results and the
      adaptive state of items the fused call does not detect for (not flagged, nb2detect <= 0) are thrown away
   4. the new points behind the frame's, lmid = nlmid + k; more than n_max keypoints: OVERFLOW; a repeated id: DUP_LMID -- both leave
      everything but the record and the adaptive state alone
   5. describeBRIEF of the new points, CameraCalibration.computeKeypoints over the whole new frame, the colour of a new point from
      cur_pyr.download(0, b) at ((int)y, (int)x)
   6. numpy.argsort by lmid, then setKeyframe + setKeyframeInfo per item
route() returns what LockstepTracker.createKeyframe returns; the GPU test holds the fused call to it byte for byte."""
import numpy as np

from ov2slam_amd import _lib as L
from tests import kfreq_ref as KF

KEYS = ("action", "n_prev", "noccupcells", "nb2detect", "n_new", "n_kf", "nb3dkps")


def empty_out(batch, n_max):
    return dict(px=np.zeros((batch, n_max, 2), np.float32), lmid=np.zeros((batch, n_max), np.int32), unpx=np.zeros((batch, n_max, 2), np.float32),
                bv=np.zeros((batch, n_max, 3), np.float64), desc=np.zeros((batch, n_max, 32), np.uint8), valid=np.zeros((batch, n_max), np.uint8),
                color=np.zeros((batch, n_max), np.uint8))


def counts(params, px, is3d):
    """noccupcells_ and nb3dkps_ of a frame with these keypoints, by the reference's own loop"""
    cur = dict(kps={i: dict(px=px[i], is3d=bool(is3d[i])) for i in range(len(px))})
    nocc, nb3d, _ = KF.replay_counts(params, cur)
    return nocc, nb3d


def route(ctx, trk, cal, n_active, px, lmid, is3d, n, make_kf, nlmid, nkfid, time, params, state, Twc=None, out=None):
    na, nm = int(n_active), trk.n_max
    out = empty_out(trk.batch, nm) if out is None else out
    fast = params["detector"] == "gridfast"
    recs = [dict.fromkeys(KEYS, 0) for _ in range(na)]
    flagged = [b for b in range(na) if make_kf[b]]
    for b in flagged:
        nocc, nb3d = counts(params, px[b, :n[b]], is3d[b, :n[b]])
        recs[b].update(n_prev=int(n[b]), noccupcells=nocc, nb3dkps=nb3d, nb2detect=params["nbmaxkps"] - nocc)
    ncur = np.array([int(n[b]) for b in range(na)], np.int32)
    desc0 = valid0 = None
    if params["use_brief"] and flagged:
        desc0, valid0 = trk.describeBRIEF(na, px[:na], ncur)
    new = [np.zeros((0, 2), np.float32)] * na
    wants = [b for b in flagged if recs[b]["nb2detect"] > 0]
    if wants and (trk.w // params["det_cell"]) * (trk.h // params["det_cell"]) > 0:
        st = np.array(state[:na], copy=True)
        if fast:
            found = trk.detectGridFAST(na, params["det_cell"], px, ncur, st, mask_mode=params["mask_mode"], subpix=params["do_subpix"])
        else:
            found = trk.detectSingleScale(na, params["det_cell"], px, ncur, params["roi"], st, subpix=params["do_subpix"])
        for b in wants:
            new[b], state[b] = found[b], st[b]
    lvl0 = {}
    for b in flagged:
        r, m0, k = recs[b], int(n[b]), len(new[b])
        r.update(n_new=k, n_kf=m0 + k)
        if m0 + k > nm:
            r["action"] = L.OV2_CKF_OVERFLOW
            continue
        ids = np.concatenate([lmid[b, :m0], nlmid[b] + np.arange(k, dtype=np.int32)]).astype(np.int32)
        if len(set(ids.tolist())) < len(ids):
            r["action"] = L.OV2_CKF_DUP_LMID
            continue
        r["action"] = L.OV2_CKF_CREATED
        pts = np.concatenate([px[b, :m0], new[b]]).astype(np.float32)
        unpx, bv = cal.computeKeypoints(pts) if len(pts) else (np.zeros((0, 2), np.float32), np.zeros((0, 3)))
        out["px"][b, :m0 + k], out["lmid"][b, :m0 + k], out["unpx"][b, :m0 + k], out["bv"][b, :m0 + k] = pts, ids, unpx, bv
        if k:
            if b not in lvl0:
                lvl0[b] = trk.cur_pyr.download(0, b)[0]
            xi = np.clip(new[b][:, 0].astype(np.int32), 0, trk.w - 1); yi = np.clip(new[b][:, 1].astype(np.int32), 0, trk.h - 1)
            out["color"][b, m0:m0 + k] = lvl0[b][yi, xi]
        if params["use_brief"]:
            out["desc"][b, :m0], out["valid"][b, :m0] = desc0[b, :m0], valid0[b, :m0]
        o = np.argsort(ids, kind="stable")
        T = trk.getPose(b) if Twc is None else np.asarray(Twc, np.float64).reshape(-1, 7)[b]
        trk.setKeyframe(b, ids[o], unpx[o], bv[o], T)
        trk.setKeyframeInfo(b, int(nkfid[b]), float(time[b]), r["nb3dkps"])
    created = [b for b in flagged if recs[b]["action"] == L.OV2_CKF_CREATED and recs[b]["n_new"] > 0]
    if params["use_brief"] and created:                                 # describeBRIEF of the new points, one call over the batch
        pts = np.zeros((na, nm, 2), np.float32); cnt = np.zeros(na, np.int32)
        for b in created:
            pts[b, :len(new[b])], cnt[b] = new[b], len(new[b])
        d1, v1 = trk.describeBRIEF(na, pts, cnt)
        for b in created:
            m0, k = recs[b]["n_prev"], recs[b]["n_new"]
            out["desc"][b, m0:m0 + k], out["valid"][b, m0:m0 + k] = d1[b, :k], v1[b, :k]
    return recs, out
