"""VisualFrontEnd::kltTrackingFromKF (src/visual_front_end.cpp:278-442 of the reference) restated on top of oracle.fb_klt, in the
style of oracle.klt_tracking: test infrastructure for the from-keyframe mode of the lock-step tracker.

Every frame is tracked from the LAST KEYFRAME: the template pyramid is kf_pyr_ (:52-54) and the source point of a keypoint is the
keyframe's px_ of its lmid_ (:336, :346).  What differs from kltTracking, by line:
  membership  a keypoint whose lmid_ the keyframe does not hold is removed before anything is tracked (:316-320, :348-351)
  priors      a keypoint without a 3-D prior starts from the frame's own px_ (:343-345), not from its source point
  retry       a 3-D-prior keypoint that the one-level pass lost is retried on the full pyramid from the frame's own px_ (:386)
  33 % rule   counted over the prior pass (:395); when it fires `vpriors = vkps` resets every prior of the second call to the
              keyframe's px (:396-400)
The reference composes its lists by push_back; keypoints are independent inside fbKltTracking, so results are reported per slot.
retry_from / noprior_from select the OTHER rule (kltTracking's) for the two starts, so that tests can show a case tells them apart."""
import numpy as np

ST_OK, ST_RETRIED, ST_NOT_IN_KF = 1, 2, 4


def join(cur_lmid, kf_lmid):
    """(in_kf (n,) bool, j (n,) index into the keyframe's arrays or -1)"""
    at = {int(v): k for k, v in enumerate(np.asarray(kf_lmid).reshape(-1))}
    j = np.array([at.get(int(v), -1) for v in np.asarray(cur_lmid).reshape(-1)], np.int64).reshape(-1)
    return j >= 0, j


def _oracle_fb(kf_pyr, cur_pyr, win, lvl, ferr, fbdist, kps, pri, max_iter, eps):
    from oracle import oracle as O
    o, st, _ = O.fb_klt(kf_pyr, cur_pyr, win, lvl, ferr, fbdist, kps, pri, max_iter, eps)
    return o, st


def klt_tracking_from_kf(kf_pyr, cur_pyr, cur_px, cur_lmid, kf_lmid, kf_px, proj, has_prior, win=9, nklt_pyr_lvl=3, ferr=30.,
                         fbdist=0.5, klt_use_prior=True, max_iter=30, eps=0.01, retry_from="cur", noprior_from="cur", fb=_oracle_fb):
    """kf_pyr / cur_pyr: oracle pyramids (or, with fb, whatever fb takes: the route of separate calls on the device passes the
    tracker's item views and a wrapper of FeatureTracker.fbKltTracking).  kf_lmid / kf_px: the keypoints the keyframe holds NOW and their px; cur_px / cur_lmid: the frame; proj /
    has_prior: the projection of every slot's map point and whether it exists and lies in the image (:326-339).
    -> (px (n, 2) float32: the value handed to updateKeypoint, or the last forward result of a lost keypoint, or the input px of one
        the keyframe does not hold; status (n,) uint8: bit 0 tracked, bit 1 went through the second call after losing the first,
        bit 2 not in the keyframe; bp3preq)"""
    cur_px = np.ascontiguousarray(cur_px, np.float32).reshape(-1, 2)
    kf_px = np.ascontiguousarray(kf_px, np.float32).reshape(-1, 2)
    proj = np.ascontiguousarray(proj, np.float32).reshape(-1, 2)
    n = len(cur_px)
    in_kf, j = join(cur_lmid, kf_lmid)
    src = np.where(in_kf[:, None], kf_px[np.maximum(j, 0)] if len(kf_px) else cur_px, cur_px).astype(np.float32).reshape(-1, 2)
    hp = np.zeros(n, bool) if (has_prior is None or not klt_use_prior) else (np.asarray(has_prior).reshape(-1) != 0)
    hp = hp & in_kf
    out = cur_px.copy()
    status = np.zeros(n, np.uint8)
    status[~in_kf] = ST_NOT_IN_KF
    p3p = False
    ia = np.nonzero(hp)[0]
    ib = [int(i) for i in np.nonzero(in_kf & ~hp)[0]]
    start = lambda i: (cur_px[i] if noprior_from == "cur" else src[i]).copy()
    pri_b = {i: start(i) for i in ib}
    if len(ia):
        o, st = fb(kf_pyr, cur_pyr, win, 1, ferr, fbdist, src[ia], proj[ia], max_iter, eps)
        st = np.asarray(st).astype(bool)
        for k, i in enumerate(ia):
            out[i] = o[k]
            if st[k]:
                status[i] = ST_OK
            else:
                ib.append(int(i))
                pri_b[int(i)] = (cur_px[i] if retry_from == "cur" else o[k]).copy()                       # :386
                status[i] = ST_RETRIED
        if st.sum() < 0.33 * len(ia):                                                                    # :395-400
            p3p = True
            for i in ib:
                pri_b[i] = src[i].copy()
    if len(ib):
        ib = np.array(ib)
        o, st = fb(kf_pyr, cur_pyr, win, nklt_pyr_lvl, ferr, fbdist, src[ib], np.stack([pri_b[int(i)] for i in ib]), max_iter, eps)
        out[ib] = o
        status[ib] |= np.asarray(st).astype(np.uint8)
    return out, status, p3p
