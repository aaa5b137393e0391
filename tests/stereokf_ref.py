"""ov2_btracker_stereo_keyframe (scope row f22) for the tests: the ROUTE of separate calls it replaces, the slot-order cell table of
its one deviation, the scenario both trackers of tests/test_gpu_stereokf.py play, and the scenario's CONDITIONS computed without a GPU.

  cell_tables()   Frame::getSurroundingKeypoints' grid with the keypoints of a cell in SLOT ORDER (the reference: vgridkps_ insertion
                  order, which the resident frame does not carry): cell (floor(px.y / cellsize), floor(px.x / cellsize)) in float32
                  as k_prior_stereo computes it, a keypoint outside the grid in no cell.
  route()         plain Python over existing calls on a tracker whose frames are resident: getFrame; state = is3d, unpx / bv by
                  computeKeypoints, the cell tables; stereo_priors_batch; stereo_match_batch_arrays on cur_pyr and the right pyramid;
                  computeKeypoints of the right camera on right_px; triangulate_keyframe_batch with src = None; updateFrame with one SET
                  op per STEREO_OK slot; setKeyframeInfo with the recounted nb3dkps.
  scenario()      per config the cameras, the parameter structs' ingredients and per item a left / right pair made as
                  tests/stereo_cases.images makes them (one texture seed per item; item 1 with the disparity REVERSED, so that true
                  matches triangulate behind the cameras), a second left image for the step that follows, a pose, and the frame that
                  setFrame installs: keypoints as stereo_cases.keypoints lays them out (interior and within 28 px of every border),
                  about 35 % of them 3-D with points on the scene's plane that project onto the true right match, about 30 % of those
                  far off.  The scene is a fronto-parallel plane at depth fx * baseline / disparity, Tcic0 a pure x-translation.
                  tri.Kr carries a focal length a few per cent off: the right reprojection error grows with the distance from the
                  principal column and crosses fmax_reproj_err at about 0.3 w, so both sides of that gate are populated.
  conditions()    what the frames of a config make the block do, from tests/priors_ref.py (flat_stereo on the slot-order table),
                  oracle.stereo_matching (as tests/stereo_cases.py: oracle_run) and tests/tri_ref.py, over the slots setFrame installs
                  (the detector's fresh points of createKeyframe are 2-D: they are nobody's 3-D neighbour and change no old slot's
                  result)."""
import ctypes as C
import functools

import numpy as np

from ov2slam_amd import _lib as L
from tests import stereo_cases as SC
from tests import tri_ref as T
from tests.match_ref import FISHEYE4, grid_width

F32 = np.float32
N_MAX, CELL, WIN, BASELINE, EMAX = 160, 35, 9, 0.11, 3.0
CONFIGS = {
    "rect":           dict(w=376, h=240, batch=4, disp=12, lvl=3, rect=True, D=None, model="pinhole", n_inner=55, n_edge=45),
    "unrect-radtan":  dict(w=376, h=240, batch=4, disp=12, lvl=3, rect=False, D=SC.RADTAN, model="pinhole", n_inner=55, n_edge=45),
    "unrect-fisheye": dict(w=161, h=121, batch=2, disp=6, lvl=1, rect=False, D=FISHEYE4, model="fisheye", n_inner=35, n_edge=25),
}
SET = L.OV2_RES_SET_POINT
NOT_REQUESTED, NOT_KEYFRAME, DONE = L.OV2_SKF_NOT_REQUESTED, L.OV2_SKF_NOT_KEYFRAME, L.OV2_SKF_DONE
REC_KEYS = tuple(f for f, _ in L.StereoKeyframeResult._fields_)      # action, n, n_prior3d, n_prior_nb, n_stereo_kps, n_stereo, n_stereo_good, nb3dkps


# ---- the slot-order cell table -------------------------------------------------------------------------------------------------------
def cell_tables(px, img_w, img_h, cellsize):
    """-> (cell_start (ncells + 1,) int32, cell_kp int32): per cell the slots of its keypoints, ascending"""
    px = np.asarray(px, F32).reshape(-1, 2)
    nbw, nbh = grid_width(dict(img_w=img_w, img_h=img_h, ncellsize=cellsize))
    cs = F32(cellsize)
    with np.errstate(all="ignore"):
        rf, cf = np.floor(px[:, 1] / cs), np.floor(px[:, 0] / cs)
        inside = (rf >= 0) & (cf >= 0) & (rf < nbh) & (cf < nbw)                      # false for NaN
    cell = np.where(inside, np.nan_to_num(rf) * nbw + np.nan_to_num(cf), -1).astype(np.int64)
    slots = np.nonzero(inside)[0]
    order = slots[np.argsort(cell[slots], kind="stable")]
    counts = np.bincount(cell[slots], minlength=nbw * nbh) if len(slots) else np.zeros(nbw * nbh, np.int64)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), order.astype(np.int32)


# ---- the route -----------------------------------------------------------------------------------------------------------------------
def se3_inverse(lib, Twc):
    """ov2_se3_inverse: the arithmetic k_ckf_install inverts the keyframe's pose with"""
    a, out = np.ascontiguousarray(Twc, np.float64), np.zeros(7)
    L.check(lib.ov2_se3_inverse(a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return out


def empty_out(batch, n_max, poison=None):
    o = dict(right_px=np.zeros((batch, n_max, 2), np.float32), stereo_ok=np.zeros((batch, n_max), np.uint8),
             tri_status=np.zeros((batch, n_max), np.uint8), wpt=np.zeros((batch, n_max, 3), np.float64),
             invdepth=np.zeros((batch, n_max), np.float64))
    if poison is not None:
        for a in o.values():
            a.view(np.uint8)[...] = poison
    return o


def route(ctx, t, right_pyr, na, actions, S, kf, out):
    """the separate calls for the items whose action is OV2_SKF_DONE.  t: the LockstepTracker; S: scenario(name) (cameras and
    settings); kf[b] = dict(id, time, Twc) of item b's resident keyframe; out: empty_out().  -> (records, out)"""
    import ov2slam_amd
    from ov2slam_amd import mapper, priors, stereo
    recs = [dict.fromkeys(REC_KEYS, 0) for _ in range(na)]
    for b in range(na):
        recs[b]["action"] = int(actions[b])
    done = [b for b in range(na) if actions[b] == DONE]
    if not done:                                                         # nothing is called, nothing is written
        return recs, out
    cfg = S["cfg"]
    cal_l, cal_r = calibrations(ctx, S)
    nm, batch = t.n_max, t.batch
    fr = {b: t.getFrame(b, from_device=True) for b in done}
    kps, unpx = np.zeros((batch, nm, 2), np.float32), np.zeros((batch, nm, 2), np.float32)
    pri, hp, nn = np.zeros((batch, nm, 2), np.float32), np.zeros((batch, nm), np.uint8), np.zeros(batch, np.int32)
    items, bvs = [], {}
    for b in done:
        f, n = fr[b], fr[b]["n"]
        u, bv = cal_l.computeKeypoints(f["px"]) if n else (np.zeros((0, 2), np.float32), np.zeros((0, 3)))
        cs, ck = cell_tables(f["px"], cfg["w"], cfg["h"], CELL)
        items.append(dict(Tcw=se3_inverse(ctx.lib, kf[b]["Twc"]), px=f["px"], unpx=u, bv=bv, wpt=f["wpt"], state=f["is3d"],
                          cell_start=None if cfg["rect"] else cs, cell_kp=None if cfg["rect"] else ck))
        kps[b, :n], unpx[b, :n], nn[b], bvs[b] = f["px"], u, n, bv
    P = priors.stereo_priors_batch(ctx, S["priors"], items)
    for b, p in zip(done, P):
        n = nn[b]
        pri[b, :n], hp[b, :n] = p["prior"], p["has_prior"]
        recs[b].update(n=int(n), n_prior3d=int(p["n_prior3d"]), n_prior_nb=int(p["n_prior_nb"]))
    ftr = ov2slam_amd.FeatureTracker(ctx, 30, 0.01)
    ok, right = stereo.stereo_match_batch_arrays(ftr, t.cur_pyr, right_pyr, na, nm, kps, unpx, pri, hp, nn, cal_r, rect=cfg["rect"],
                                                 Frl=None if cfg["rect"] else SC.F_XTRANS, nklt_win_size=WIN, nklt_pyr_lvl=cfg["lvl"])
    kfs = []
    for b in done:
        n = nn[b]
        ru, rbv = cal_r.computeKeypoints(right[b, :n]) if n else (np.zeros((0, 2), np.float32), np.zeros((0, 3)))
        kfs.append(dict(Twc=kf[b]["Twc"], unpx=unpx[b, :n], bv=bvs[b], is_stereo=(ok[b, :n] & (fr[b]["is3d"] == 0)).astype(np.uint8),
                        runpx=ru, rbv=rbv))
    R = mapper.triangulate_keyframe_batch(ctx, S["tri"], kfs)
    ops = [[] for _ in range(na)]
    for b, r in zip(done, R):
        n, f = nn[b], fr[b]
        out["right_px"][b, :n], out["stereo_ok"][b, :n] = right[b, :n], ok[b, :n]
        out["tri_status"][b, :n], out["wpt"][b, :n], out["invdepth"][b, :n] = r["status"], r["wpt"], r["invdepth"]
        good = (r["status"] & L.OV2_TRI_STEREO_OK) != 0
        ops[b] = [(int(f["lmid"][i]), SET, r["wpt"][i]) for i in np.nonzero(good)[0]]
        recs[b].update(n_stereo_kps=int(ok[b, :n].sum()), n_stereo=int(r["counts"]["n_stereo"]), n_stereo_good=int(r["counts"]["n_stereo_good"]),
                       nb3dkps=int(((f["is3d"] != 0) | good).sum()))
    upd = t.updateFrame(na, ops)
    for b in done:
        assert upd[b]["n_set"] == len(ops[b]) and upd[b]["n_missing"] == 0 and upd[b]["n_after"] == nn[b]
        t.setKeyframeInfo(b, kf[b]["id"], kf[b]["time"], recs[b]["nb3dkps"])
    return recs, out


# ---- the scenario --------------------------------------------------------------------------------------------------------------------
def camera(cfg):
    w, h = cfg["w"], cfg["h"]
    K = (0.61 * w, 0.608 * w, 0.488 * w, 0.517 * h)                      # tests/stereo_cases.py: case()
    return K, np.linalg.inv(np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1.0]]))


def calibrations(ctx, S):
    """(left, right) CameraCalibration: identical cameras"""
    import ov2slam_amd
    cfg, K = S["cfg"], S["K"]
    mk = lambda: ov2slam_amd.CameraCalibration(ctx, cfg["model"], *K, D=cfg["D"])
    return mk(), mk()


def pair(cfg, b, shift=(0, 0)):
    """item b's left / right pair as stereo_cases.images cuts it (seed 500 + b), the disparity reversed for item 1; shift moves both
    crops: the frame after"""
    from ov2slam_amd import synth
    w, h = cfg["w"], cfg["h"]
    d = -cfg["disp"] if b == 1 else cfg["disp"]
    tex = synth.base_texture(max(w, h) + 400, 500 + b)
    y0, x0 = 50 + shift[1], 100 + shift[0]
    l = tex[y0:y0 + h, x0:x0 + w].astype(np.uint8)
    r = tex[y0:y0 + h, x0 + d:x0 + d + w].astype(np.uint8)
    c0, c1 = w // 3, w // 3 + w // 4
    r[:, c0:c1] = np.roll(r[:, c0:c1], 3, axis=0)
    return np.ascontiguousarray(l), np.ascontiguousarray(r)


def _quat_pose(rng):
    q = np.concatenate([rng.normal(0, 0.05, 3), [1.0]])
    return np.concatenate([rng.normal(0, 0.5, 3), q / np.linalg.norm(q)])


def _rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def make_frame(cfg, K, iK, Twc, n_inner, n_edge, first_id, seed, p3d=0.35, pfar=0.30):
    """a frame for setFrame: stereo_cases.keypoints, ids first_id .. in a random slot order; a share p3d of the slots 3-D with the
    point of the scene's plane behind the pixel (float64 algebra on the undistorted pinhole ray: the generator only needs to be
    close), a share pfar of those moved so that they project 8 .. 16 px right of and 5 .. 10 px above the true match"""
    rng = np.random.default_rng(seed)
    n = n_inner + n_edge
    px = SC.keypoints(cfg["w"], cfg["h"], n_inner, n_edge, rng) if n else np.zeros((0, 2), np.float32)
    is3d = (rng.random(n) < p3d).astype(np.uint8) if 0 < p3d < 1 else np.full(n, int(p3d >= 1), np.uint8)
    far = (is3d != 0) & (rng.random(n) < pfar)
    z0 = K[0] * BASELINE / cfg["disp"]
    tgt = px.astype(np.float64)
    tgt[far] += np.stack([rng.uniform(8, 16, n), -rng.uniform(5, 10, n)], 1)[far]
    ray = (iK @ np.concatenate([tgt, np.ones((n, 1))], 1).T).T
    Pc = ray * z0
    wpt = (_rot(Twc[3:]) @ Pc.T).T + Twc[:3]
    wpt[is3d == 0] = 0.0
    return dict(n=n, px=px, lmid=(first_id + rng.permutation(n)).astype(np.int32), is3d=is3d, wpt=wpt, far=far)


@functools.lru_cache(maxsize=None)
def scenario(name):
    cfg = CONFIGS[name]
    K, iK = camera(cfg)
    w, h, B = cfg["w"], cfg["h"], cfg["batch"]
    Tcic0 = (-BASELINE, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
    Tlr = (BASELINE, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
    Kr = (K[0] * (1.0 + EMAX / (0.3 * w)), K[1], K[2], K[3])
    tri = dict(stereo=True, rect=cfg["rect"], fmax_reproj_err=EMAX, K=K, iK=iK.reshape(9), Kr=Kr, Tlr=np.array(Tlr), Tcic0=np.array(Tcic0))
    pri = dict(model=cfg["model"], K=K, D=cfg["D"], img_w=float(w), img_h=float(h), ncellsize=CELL, rect=cfg["rect"], Tcic0=Tcic0)
    items = []
    for b in range(B):
        rng = np.random.default_rng(900 + b)
        Twc = _quat_pose(rng)
        l, r = pair(cfg, b)
        # item 1: the reversed pair, few 3-D points (they project left of the keypoint, its matches lie right); item 2: none 3-D
        p3d = {1: 0.10, 2: 0.0}.get(b, 0.35)
        items.append(dict(left=l, right=r, left2=pair(cfg, b, (2, 1))[0], Twc=Twc,
                          frame=make_frame(cfg, K, iK, Twc, cfg["n_inner"], cfg["n_edge"], 0, 40 + b, p3d=p3d)))
    return dict(name=name, cfg=cfg, K=K, iK=iK, Tcic0=Tcic0, tri=tri, priors=pri, items=items)


def skf_params(ctx, S):
    """the ov2_stereo_keyframe_params of a scenario"""
    from ov2slam_amd import mapper
    cfg = S["cfg"]
    return mapper.stereo_keyframe_params(calibrations(ctx, S)[1], S["tri"], img_w=cfg["w"], img_h=cfg["h"], Tcic0=S["Tcic0"], rect=cfg["rect"],
                                         Frl=None if cfg["rect"] else SC.F_XTRANS, ncellsize=CELL, nklt_win_size=WIN, nklt_pyr_lvl=cfg["lvl"])


# ---- the conditions, without a GPU -----------------------------------------------------------------------------------------------------
def _reject_reason(P, unpx, bv, runpx, rbv):
    """why Mapper::triangulateStereo's loop body (tests/tri_ref.py: stereo_point) refuses a stereo keypoint, or None"""
    D = T.D
    Tlr, Tcic0 = T.pose(P["Tlr"]), T.pose(P["Tcic0"])
    Trl = T.se3_inv(Tlr)
    with np.errstate(all="ignore"):
        if P["rect"]:
            disp = F32(F32(unpx[0]) - F32(runpx[0]))
            if disp < 0.:
                return "negative_disparity"
            z = F32(D(P["K"][0]) * T.norm3(Tcic0[0]) / D(np.abs(disp)))
            iK = [D(v) for v in P["iK"]]
            v = (D(F32(unpx[0])), D(F32(unpx[1])), D(1))
            left = tuple((D(z) * iK[3 * i] * v[0] + D(z) * iK[3 * i + 1] * v[1]) + D(z) * iK[3 * i + 2] * v[2] for i in range(3))
        else:
            left = T.triangulate2(T.rotation_matrix(Tlr[1]), Tlr[0], bv, rbv)
        right = T.se3_act(Trl, left)
        if left[2] < 0.1 or right[2] < 0.1:
            return "depth"
        ldist = F32(T.pt_dist(T.project(P["K"], left), unpx))
        rdist = F32(T.pt_dist(T.project(P["Kr"], T.se3_act(Tcic0, left)), runpx))
        if ldist > F32(P["fmax_reproj_err"]) or rdist > F32(P["fmax_reproj_err"]):
            return "reprojection"
    return None


@functools.lru_cache(maxsize=None)
def conditions(name):
    """-> per item a dict of the populations below, over the slots setFrame installs"""
    from oracle import oracle as O
    from tests import priors_ref as PR
    S = scenario(name)
    cfg, K, iK = S["cfg"], S["K"], S["iK"]
    model = O.CAM_FISHEYE if cfg["model"] == "fisheye" else O.CAM_PINHOLE
    lvl = cfg["lvl"]
    res = []
    for it in S["items"]:
        f = it["frame"]
        n, px, is3d = f["n"], f["px"], f["is3d"]
        unpx, bv = O.compute_keypoints(model, K, cfg["D"], iK, px)
        cs, ck = cell_tables(px, cfg["w"], cfg["h"], CELL)
        Tcw = T._inv7(it["Twc"])
        pri = PR.flat_stereo(S["priors"], dict(Tcw=Tcw, px=px, unpx=unpx, bv=bv, wpt=f["wpt"], state=is3d, cell_start=cs, cell_kp=ck))
        hp = pri["has_prior"]
        opl, opr = O.Pyramid(it["left"], WIN, SC.MAX_LEVEL), O.Pyramid(it["right"], WIN, SC.MAX_LEVEL)
        p3 = {int(i): (pri["prior"][i, 0], pri["prior"][i, 1]) for i in np.nonzero(hp)[0]}
        Frl = None if cfg["rect"] else SC.F_XTRANS
        ok, right_px = O.stereo_matching(opl, opr, px, unpx, model, K, cfg["D"], cfg["rect"], Frl=Frl, win=WIN, nklt_pyr_lvl=lvl, priors3d=p3)
        d = dict(n=n, prior1=int((hp == 1).sum()), prior2=int((hp == 2).sum()), sad_accepted=0, sad_rejected=0)
        i3 = np.nonzero(hp)[0]
        first_ok = np.zeros(n, bool)
        if len(i3):
            first_ok[i3] = O.fb_klt(opl, opr, WIN, 1, 30., 0.5, px[i3], pri["prior"][i3])[1]
        d["retried"] = int(((hp != 0) & ~first_ok).sum())
        if cfg["rect"]:
            up = F32(2.0 ** lvl)
            x = O.line_min_sad(opl.level(lvl)[0], opr.level(lvl)[0], px * (F32(1.0) / up), SC.SAD_WIN, True)[0] * up
            use = (x >= 0) & (x <= px[:, 0]) & (hp == 0)
            d["sad_accepted"], d["sad_rejected"] = int(use.sum()), int(((hp == 0) & ~use).sum())
        tracked = (right_px != 0).any(axis=1)
        d["gate_rejected"], d["stereo_ok"] = int((tracked & ~ok).sum()), int(ok.sum())
        d["matched_3d"] = int((ok & (is3d != 0)).sum())                   # is3d keypoints that match: not triangulated
        runpx, rbv = O.compute_keypoints(model, K, cfg["D"], iK, right_px)
        is_stereo = ok & (is3d == 0)
        status = T.keyframe(S["tri"], dict(Twc=it["Twc"], unpx=unpx, bv=bv, is_stereo=is_stereo, runpx=runpx, rbv=rbv,
                                           src=np.full(n, -1, np.int32)))[0]
        d["tri_ok"] = int(((status & L.OV2_TRI_STEREO_OK) != 0).sum())
        reasons = [_reject_reason(S["tri"], unpx[i], bv[i], runpx[i], rbv[i]) for i in np.nonzero(is_stereo)[0]]
        assert sum(r is None for r in reasons) == d["tri_ok"]
        for k in ("negative_disparity", "depth", "reprojection"):
            d[k] = reasons.count(k)
        res.append(d)
    return tuple(res)
