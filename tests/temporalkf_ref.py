"""ov2_btracker_temporal_keyframe (scope row f23) for the tests: a plain map model, the anchor-table rule, the route of separate calls
the call replaces, and the scripted run all of them play.

  MapModel        (a) what the reference's map knows, in plain Python: lmid -> set of observing kfids and is3d, keyframes by id with
                  their keypoints (lmid -> unpx, bv) and poses.  candidates() selects by Mapper::triangulateTemporal's own rule
                  (src/mapper.cpp:238-295): the 2-D keypoints of the new keyframe whose map point is not 3-D, has two observers or more,
                  whose FIRST observer (*co_kf_ids.begin()) is another keyframe the map still holds, which holds the keypoint.
  AnchorTable     (b) the rule of the tracker's anchor table: per keypoint of the latest keyframe {lmid, kfid, unpx, bv}, per
                  keyframe referred to {kfid, Twc}; advance() at a new keyframe (inherit or anchor here, drop the rows nobody refers
                  to, append this keyframe's row, None on more than n_src_max rows, unchanged when the newest row is this keyframe),
                  set_poses() (local BA), from_map() (the caller's walk after its map culled a keyframe).
  tri_inputs()    the arrays of ov2_tri_keyframe for a frame, its keyframe and a table: the join of the slots against the keyframe,
                  src / src_unpx / src_bv from the anchors, src = -1 for 3-D slots and anchors at this keyframe.
  route()         (c) the separate calls on a tracker whose frames are resident: getFrame, the host anchor walk (AnchorTable),
                  triangulate_keyframe_batch, updateFrame with one SET op per TEMPORAL_OK slot, setKeyframe with the keyframe
                  compacted by the REMOVE_OBS slots, setKeyframeInfo, and setAnchors with the table the walk produced.
  script()        per config the camera and, per item, six keyframes of one synthetic scene: poses moving sideways (item 1 stands
                  still between keyframes 1 and 2), world points with a birth keyframe and a death, and per observation a pixel:
                  the exact projection, or one moved on purpose --
                    `once`   40 .. 50 px along the motion at the keyframe after the birth only: the rays diverge, the depth gate
                             rejects with more than 20 px of parallax (REMOVE_OBS), and the next keyframe triangulates it
                    `far`    60 .. 100 m away and 4 px along the motion: the depth gate rejects with little parallax
                    `perp`   12 px across the motion: the reprojection gate rejects
                    `init3d` 3-D from the start
                  Item 3 carries the sizes: no slot, one slot, every slot 3-D.
  simulate()      the script on the CPU with tests/tri_ref.py as the triangulation: (a) and (b) side by side, every event of the
                  script (a second call on keyframe 1, a BA pose change before keyframe 2, a culled keyframe and set_anchors before
                  keyframe 4)."""
import functools

import numpy as np

from ov2slam_amd import _lib as L
from tests import match_ref as MR
from tests import tri_ref as T

F32 = np.float32
N_MAX, N_SRC_MAX, EMAX = 160, 8, 3.0
N_KF = 6
NOT_REQUESTED, NOT_KEYFRAME, DONE, SRC_OVERFLOW = L.OV2_TKF_NOT_REQUESTED, L.OV2_TKF_NOT_KEYFRAME, L.OV2_TKF_DONE, L.OV2_TKF_SRC_OVERFLOW
TRIED, OK, NO_MOTION, REMOVE_OBS = L.OV2_TRI_TEMPORAL_TRIED, L.OV2_TRI_TEMPORAL_OK, L.OV2_TRI_NO_MOTION, L.OV2_TRI_REMOVE_OBS
REC_KEYS = tuple(f for f, _ in L.TemporalKeyframeResult._fields_)  # action n n_candidates n_temporal_good n_remove_obs n_no_motion nb3dkps n_rows
CONFIGS = {
    "mono-pinhole":   dict(w=376, h=240, batch=4, D=None, model="pinhole", stereo=False, disp=12, lvl=3, rect=True, n_inner=0, n_edge=0),
    "stereo-fisheye": dict(w=161, h=121, batch=4, D=MR.FISHEYE4, model="fisheye", stereo=True, disp=6, lvl=1, rect=False, n_inner=0, n_edge=0),
}


def kfid_of(k, b):
    return 100 * (k + 1) + b


# ---- (a) the map ---------------------------------------------------------------------------------------------------------------------
class MapModel:
    def __init__(self):
        self.obs, self.is3d, self.kfs = {}, {}, {}

    def add_keyframe(self, kfid, Twc, lmid, unpx, bv, is3d):
        """MapManager::addKeyframe: the keyframe with its keypoints, one observation per keypoint"""
        self.kfs[kfid] = dict(Twc=np.array(Twc, np.float64), kps={int(l): (np.array(u, F32), np.array(v, np.float64)) for l, u, v in zip(lmid, unpx, bv)})
        for l, d in zip(lmid, is3d):
            self.obs.setdefault(int(l), set()).add(kfid)
            self.is3d[int(l)] = bool(self.is3d.get(int(l), False) or d)

    def candidates(self, kfid):
        """lmid -> source kfid for the 2-D keypoints of keyframe `kfid` that reach :297 (before the no-motion skip of :287, which the
        triangulation itself takes)"""
        out = {}
        for lm in self.kfs[kfid]["kps"]:
            if self.is3d[lm]:                                             # :250 (getKeypoints2d: the frame's 2-D keypoints)
                continue
            co = self.obs[lm]
            if len(co) < 2:                                               # :258
                continue
            first = min(co)                                               # :262
            if first == kfid or first not in self.kfs:                    # :264, :271
                continue
            if lm not in self.kfs[first]["kps"]:                          # :293
                continue
            out[lm] = first
        return out

    def remove_obs(self, lm, kfid):
        """MapManager::removeMapPointObs"""
        self.obs[lm].discard(kfid)
        self.kfs[kfid]["kps"].pop(lm, None)

    def update_point(self, lm):
        self.is3d[lm] = True

    def cull(self, kfid):
        """MapManager::removeKeyframe: the keyframe and its observations"""
        for lm in self.kfs.pop(kfid)["kps"]:
            self.obs[lm].discard(kfid)


# ---- (b) the anchor table -------------------------------------------------------------------------------------------------------------
class AnchorTable:
    def __init__(self, lmid=(), kfid=(), unpx=None, bv=None, row_kfid=(), row_Twc=None):
        self.lmid, self.kfid = np.array(lmid, np.int32).reshape(-1), np.array(kfid, np.int32).reshape(-1)
        n, r = len(self.lmid), len(row_kfid)
        self.unpx = np.zeros((0, 2), F32) if unpx is None else np.array(unpx, F32).reshape(n, 2)
        self.bv = np.zeros((0, 3)) if bv is None else np.array(bv, np.float64).reshape(n, 3)
        self.row_kfid = np.array(row_kfid, np.int32).reshape(-1)
        self.row_Twc = np.zeros((0, 7)) if row_Twc is None else np.array(row_Twc, np.float64).reshape(r, 7)

    def advance(self, kfid, Twc, kf_lmid, kf_unpx, kf_bv, n_src_max):
        """the table at the new keyframe (kf_lmid ascending) -> AnchorTable, or None when more than n_src_max rows stay referred to"""
        if len(self.row_kfid) and self.row_kfid[-1] == kfid:
            return self
        old = {int(l): i for i, l in enumerate(self.lmid)}
        hit = np.array([old.get(int(l), -1) for l in kf_lmid], np.int64).reshape(-1)
        kf = np.where(hit >= 0, self.kfid[hit] if len(self.kfid) else 0, kfid).astype(np.int32) if len(hit) else np.zeros(0, np.int32)
        live = [int(k) for k in self.row_kfid if (kf[hit >= 0] == k).any()] if len(hit) else []
        if len(live) + 1 > n_src_max:
            return None
        unpx = np.array(kf_unpx, F32).reshape(-1, 2).copy()
        bv = np.array(kf_bv, np.float64).reshape(-1, 3).copy()
        if (hit >= 0).any():
            unpx[hit >= 0], bv[hit >= 0] = self.unpx[hit[hit >= 0]], self.bv[hit[hit >= 0]]
        rows = {int(k): self.row_Twc[i] for i, k in enumerate(self.row_kfid)}
        return AnchorTable(kf_lmid, kf, unpx, bv, live + [kfid], [rows[k] for k in live] + [np.array(Twc, np.float64)])

    def set_poses(self, pairs):
        """(kfid, Twc) pairs -> the number that anchor nothing"""
        ignored = 0
        for kfid, Twc in pairs:
            at = np.nonzero(self.row_kfid == kfid)[0]
            if len(at):
                self.row_Twc[at[0]] = Twc
            else:
                ignored += 1
        return ignored

    @staticmethod
    def from_map(M, lmids):
        """the caller's walk over its map for the ids an item's table holds: the first observer the map still has; an id without
        one leaves the table"""
        rec = []
        for lm in sorted(int(l) for l in lmids):
            co = [k for k in M.obs.get(lm, ()) if k in M.kfs and lm in M.kfs[k]["kps"]]
            if co:
                k = min(co)
                rec.append((lm, k) + M.kfs[k]["kps"][lm])
        rows = sorted({r[1] for r in rec})
        return AnchorTable([r[0] for r in rec], [r[1] for r in rec], [r[2] for r in rec] or None, [r[3] for r in rec] or None, rows,
                           [M.kfs[k]["Twc"] for k in rows] or None)

    def as_dict(self, inv):
        """what LockstepTracker.getAnchors returns (inv: the inverse the library computes)"""
        return dict(n=len(self.lmid), lmid=self.lmid, kfid=self.kfid, unpx=self.unpx, bv=self.bv, n_rows=len(self.row_kfid), row_kfid=self.row_kfid,
                    row_Twc=self.row_Twc, row_Tcw=np.array([inv(T_) for T_ in self.row_Twc]).reshape(-1, 7))


def tri_inputs(frame, kf, table, inv):
    """frame: dict(n, lmid, is3d); kf: dict(id, Twc, lmid ascending, unpx, bv); table: the AnchorTable AFTER advance(); inv: a pose's
    inverse -> the dict mapper.triangulate_keyframe_batch takes, and src_kfid (n,) (-1: no candidate)"""
    n = frame["n"]
    at_kf = {int(l): i for i, l in enumerate(kf["lmid"])}
    at_tb = {int(l): i for i, l in enumerate(table.lmid)}
    row_of = {int(k): i for i, k in enumerate(table.row_kfid)}
    unpx, bv = np.zeros((n, 2), F32), np.zeros((n, 3))
    src, sun, sbv, skf = np.full(n, -1, np.int32), np.zeros((n, 2), F32), np.zeros((n, 3)), np.full(n, -1, np.int32)
    for i in range(n):
        lm = int(frame["lmid"][i])
        j = at_kf.get(lm, -1)
        if j < 0:
            continue
        unpx[i], bv[i] = kf["unpx"][j], kf["bv"][j]
        e = at_tb.get(lm, -1)
        if e < 0:
            continue
        sun[i], sbv[i] = table.unpx[e], table.bv[e]
        k = int(table.kfid[e])
        if k != kf["id"] and not frame["is3d"][i]:
            src[i], skf[i] = row_of[k], k
    rows = table.row_Twc.reshape(-1, 7)
    d = dict(Twc=np.array(kf["Twc"], np.float64), unpx=unpx, bv=bv, src=src, src_unpx=sun, src_bv=sbv, src_Twc=rows,
             src_Tcw=np.array([inv(T_) for T_ in rows]).reshape(-1, 7))
    return d, skf


# ---- (c) the route -------------------------------------------------------------------------------------------------------------------
def empty_out(batch, n_max, poison=None):
    o = dict(tri_status=np.zeros((batch, n_max), np.uint8), wpt=np.zeros((batch, n_max, 3), np.float64),
             invdepth=np.zeros((batch, n_max), np.float64), src_kfid=np.zeros((batch, n_max), np.int32))
    if poison is not None:
        for a in o.values():
            a.view(np.uint8)[...] = poison
    return o


def se3_inverse(lib, Twc):
    import ctypes as C
    a, out = np.ascontiguousarray(Twc, np.float64), np.zeros(7)
    L.check(lib.ov2_se3_inverse(a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return out


def route(ctx, t, na, actions, tri, n_src_max, kf, tables, out):
    """the separate calls for the items whose action is OV2_TKF_DONE.  t: the LockstepTracker; tri: the ov2_tri_params dict; kf[b] =
    dict(id, time, Twc, lmid ascending, unpx, bv) of item b's resident keyframe (compacted in place); tables[b]: item b's AnchorTable
    (replaced); out: empty_out().  -> (records, out)"""
    from ov2slam_amd import mapper
    recs = [dict.fromkeys(REC_KEYS, 0) for _ in range(na)]
    for b in range(na):
        recs[b]["action"] = int(actions[b])
    inv = lambda T_: se3_inverse(ctx.lib, T_)
    done, fr, kfs, skfs = [], {}, [], {}
    for b in range(na):
        if actions[b] != DONE:
            continue
        nt = tables[b].advance(kf[b]["id"], kf[b]["Twc"], kf[b]["lmid"], kf[b]["unpx"], kf[b]["bv"], n_src_max)
        if nt is None:                                                    # the walk finds too many source keyframes: nothing is called
            recs[b]["action"] = SRC_OVERFLOW
            continue
        tables[b] = nt
        fr[b] = t.getFrame(b, from_device=True)
        d, skfs[b] = tri_inputs(fr[b], kf[b], nt, inv)
        done.append(b)
        kfs.append(d)
    if not done:
        return recs, out
    R = mapper.triangulate_keyframe_batch(ctx, tri, kfs)
    ops = [[] for _ in range(na)]
    for b, r in zip(done, R):
        f, n, st = fr[b], fr[b]["n"], r["status"]
        out["tri_status"][b, :n], out["wpt"][b, :n], out["invdepth"][b, :n], out["src_kfid"][b, :n] = st, r["wpt"], r["invdepth"], skfs[b]
        good = (st & OK) != 0
        ops[b] = [(int(f["lmid"][i]), L.OV2_RES_SET_POINT, r["wpt"][i]) for i in np.nonzero(good)[0]]
        recs[b].update(n=int(n), n_candidates=int(r["counts"]["n_candidates"]), n_temporal_good=int(r["counts"]["n_temporal_good"]),
                       n_remove_obs=int(((st & REMOVE_OBS) != 0).sum()), n_no_motion=int(((st & NO_MOTION) != 0).sum()),
                       nb3dkps=int(((f["is3d"] != 0) | good).sum()), n_rows=len(tables[b].row_kfid))
    upd = t.updateFrame(na, ops)
    for b, r in zip(done, R):
        assert upd[b]["n_set"] == len(ops[b]) and upd[b]["n_missing"] == 0 and upd[b]["n_after"] == fr[b]["n"]
        gone = set(int(l) for l in fr[b]["lmid"][(r["status"] & REMOVE_OBS) != 0])
        if gone:
            keep = np.array([int(l) not in gone for l in kf[b]["lmid"]], bool)
            kf[b].update(lmid=kf[b]["lmid"][keep], unpx=kf[b]["unpx"][keep], bv=kf[b]["bv"][keep])
            t.setKeyframe(b, kf[b]["lmid"], kf[b]["unpx"], kf[b]["bv"], kf[b]["Twc"])
        t.setKeyframeInfo(b, kf[b]["id"], kf[b]["time"], recs[b]["nb3dkps"])
        tb = tables[b]
        t.setAnchors(b, tb.lmid, tb.kfid, tb.unpx, tb.bv, tb.row_kfid, tb.row_Twc)
    return recs, out


# ---- the script ----------------------------------------------------------------------------------------------------------------------
def camera(cfg):
    w, h = cfg["w"], cfg["h"]
    K = (0.61 * w, 0.608 * w, 0.488 * w, 0.517 * h)
    return K, np.linalg.inv(np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1.0]]))


def _rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _pose(b, k):
    """keyframe k of item b: 0.3 m to the right per keyframe and a slow yaw; item 1 stands still (5 mm) from keyframe 1 to 2"""
    step = np.array([0.30, 0.02, 0.04])
    t = np.array([0.1 * b, -0.05 * b, 0.0]) + step * k
    if b == 1 and k >= 2:
        t = t - step + np.array([0.005, 0.0, 0.0])
    a = 0.004 * k + 0.01 * b
    q = np.array([0.002 * b, np.sin(a / 2), 0.001 * k, np.cos(a / 2)])
    return np.concatenate([t, q / np.linalg.norm(q)])


def _project(cfg, K, Pc):
    """the pixel of a camera-frame point through the camera's forward model, float32"""
    x, y = Pc[0] / Pc[2], Pc[1] / Pc[2]
    if cfg["D"] is None:
        return np.array([K[0] * x + K[2], K[1] * y + K[3]], F32)
    u, v = MR.distort(dict(K=K, D=cfg["D"], model=cfg["model"]), np.float64(x), np.float64(y))
    return np.array([u, v], F32)


KINDS = ("clean", "once", "far", "perp", "init3d")


@functools.lru_cache(maxsize=None)
def script(name):
    """-> dict(cfg, K, iK, tri, items); items[b] = dict(poses (N_KF, 7), frames[k] = dict(px, lmid, kind), init_wpt {lmid: xyz})"""
    cfg = CONFIGS[name]
    K, iK = camera(cfg)
    w, h, B = cfg["w"], cfg["h"], cfg["batch"]
    base = 0.11
    tri = dict(stereo=cfg["stereo"], rect=cfg["rect"], fmax_reproj_err=EMAX, K=K, iK=iK.reshape(9), Kr=K, Tlr=np.array([base, 0, 0, 0, 0, 0, 1.0]),
               Tcic0=np.array([-base, 0, 0, 0, 0, 0, 1.0]))
    items = []
    for b in range(B):
        rng = np.random.default_rng(7000 + b)
        poses = np.array([_pose(b, k) for k in range(N_KF)])
        pts = []                                                           # (lmid, birth, last, kind, world point)
        lm = 0
        for kb in range(N_KF):
            for _ in range(40 if kb == 0 else 14):
                kind = KINDS[int(rng.choice(len(KINDS), p=[0.5, 0.15, 0.1, 0.15, 0.1]))]
                z = rng.uniform(60, 100) if kind == "far" else rng.uniform(2.5, 7.0)
                u = np.array([rng.uniform(0.1 * w, 0.9 * w), rng.uniform(0.1 * h, 0.9 * h), 1.0])
                Pc = (iK @ u) * z
                X = _rot(poses[kb][3:]) @ Pc + poses[kb][:3]
                life = int(rng.integers(0, 5))                             # keyframes after the birth; `once` needs two
                pts.append((lm, kb, kb + (max(life, 2) if kind == "once" else life), kind, X))
                lm += 1
        frames, init_wpt, dead = [], {}, set()                           # a point that left the frame never comes back
        for k in range(N_KF):
            px, ids, kinds = [], [], []
            motion = _rot(poses[k][3:]).T @ np.array([1.0, 0.0, 0.0])      # the direction image points move against, in this camera
            along = -motion[:2] / np.linalg.norm(motion[:2])
            across = np.array([-along[1], along[0]])
            for (l, kb, kl, kind, X) in pts:
                if not (kb <= k <= kl) or l in dead:
                    continue
                Pc = _rot(poses[k][3:]).T @ (X - poses[k][:3])
                if Pc[2] < 0.5:
                    dead.add(l)
                    continue
                Pm = Pc.copy()
                if k > kb:                                                 # the moved observations, in normalised coordinates
                    d = np.zeros(2)
                    if kind == "once" and k == kb + 1:
                        d = -along * rng.uniform(40, 50)
                    elif kind == "far":
                        d = -along * 4.0
                    elif kind == "perp":
                        d = across * 12.0 * (w / 376.0)
                    Pm[:2] = Pc[:2] + d / np.array([K[0], K[1]]) * Pc[2]
                p = _project(cfg, K, Pm)
                if not (4 <= p[0] < w - 4 and 4 <= p[1] < h - 4):
                    dead.add(l)
                    continue
                px.append(p); ids.append(l); kinds.append(kind)
                if kind == "init3d":
                    init_wpt[l] = X
            order = rng.permutation(len(ids))[:N_MAX]
            frames.append(dict(px=np.array(px, F32).reshape(-1, 2)[order], lmid=np.array(ids, np.int32)[order], kind=[kinds[i] for i in order]))
        if b == 3:                                                         # the sizes: no slot, one 2-D slot, every slot 3-D
            f2 = frames[2]
            all3d = [i for i, kd in enumerate(f2["kind"]) if kd == "init3d"]
            one = [i for i, kd in enumerate(frames[1]["kind"]) if kd == "clean"][:1]
            pick = lambda f, ii: dict(px=f["px"][ii], lmid=f["lmid"][ii], kind=[f["kind"][i] for i in ii])
            frames = [pick(frames[0], []), pick(frames[1], one), pick(f2, all3d)] + [pick(frames[k], [i for i, kd in enumerate(frames[k]["kind"]) if kd == "init3d"])
                                                                                    for k in range(3, N_KF)]
        items.append(dict(poses=poses, frames=frames, init_wpt=init_wpt))
    return dict(name=name, cfg=cfg, K=K, iK=iK, tri=tri, items=items, Tcic0=tuple(tri["Tcic0"]))


def frame_for(item, k, known):
    """the frame setFrame installs at keyframe k: the script's pixels and ids, 3-D where `known` (lmid -> wpt, the points made so
    far) or the script's init3d says so"""
    f = item["frames"][k]
    n = len(f["lmid"])
    is3d, wpt = np.zeros(n, np.uint8), np.zeros((n, 3))
    for i, l in enumerate(f["lmid"]):
        X = known.get(int(l), item["init_wpt"].get(int(l)))
        if X is not None:
            is3d[i], wpt[i] = 1, X
    return dict(n=n, px=f["px"], lmid=f["lmid"], is3d=is3d, wpt=wpt)


# ---- the script on the CPU -----------------------------------------------------------------------------------------------------------
def _inv(T_):
    t, q = T.se3_inv(T.pose(T_))
    return np.array(list(t) + list(q), np.float64)


def keyframe_of(S, frame, kfid, Twc):
    """createKeyframe without a detector for an undistorted pinhole camera: unpx = px, bv = iK (x, y, 1) normalised, sorted by lmid"""
    assert S["cfg"]["D"] is None
    o = np.argsort(frame["lmid"], kind="stable")
    px = frame["px"][o].astype(F32)
    ray = (S["iK"] @ np.concatenate([px.astype(np.float64), np.ones((len(px), 1))], 1).T).T
    return dict(id=kfid, Twc=np.array(Twc, np.float64), lmid=frame["lmid"][o].copy(), unpx=px, bv=ray / np.maximum(np.linalg.norm(ray, axis=1, keepdims=True), 1e-300))


def reject_reason(P, Twc, unpx, bv, src_Twc, src_Tcw, kfunpx, kfbv):
    """why tri_ref.temporal_point does not make a point, from its own pieces -> ('depth' | 'reproj' | None, parallax)"""
    Tcicj = T.se3_mul(T.pose(src_Tcw), T.pose(Twc))
    R = T.rotation_matrix(Tcicj[1])
    parallax = float(T.pt_dist(kfunpx, T.project(P["K"], T.matvec(R, tuple(np.float64(v) for v in bv)))))
    left = T.triangulate2(R, Tcicj[0], kfbv, bv)
    right = T.se3_act(T.se3_inv(Tcicj), left)
    if left[2] < 0.1 or right[2] < 0.1:
        return "depth", parallax
    ld, rd = F32(T.pt_dist(T.project(P["K"], left), kfunpx)), F32(T.pt_dist(T.project(P["K"], right), unpx))
    return ("reproj" if ld > F32(P["fmax_reproj_err"]) or rd > F32(P["fmax_reproj_err"]) else None), parallax


def simulate(name, b, stereo=None, n_src_max=N_SRC_MAX):
    """item b of the script on the CPU -> the log: one entry per call, dict(k, tag, a (lmid -> source kfid by the map), b (the same by
    the table), same_src (unpx and bv agree for every candidate), status {lmid: bits}, reason {lmid: (why, parallax)}, n_not_in_kf,
    n_3d, rows)"""
    S = script(name)
    P = dict(S["tri"], stereo=S["cfg"]["stereo"] if stereo is None else stereo)
    item = S["items"][b]
    M, tb, known, log = MapModel(), AnchorTable(), {}, []
    poses = item["poses"].copy()

    def call(k, kf, frame, tag):
        nonlocal tb
        A = M.candidates(kf["id"])
        tb = tb.advance(kf["id"], kf["Twc"], kf["lmid"], kf["unpx"], kf["bv"], n_src_max)
        assert tb is not None
        d, skf = tri_inputs(frame, kf, tb, _inv)
        Bc = {int(frame["lmid"][i]): int(skf[i]) for i in range(frame["n"]) if skf[i] >= 0}
        same = all(np.array_equal(d["src_unpx"][i], M.kfs[A[int(l)]]["kps"][int(l)][0]) and np.array_equal(d["src_bv"][i], M.kfs[A[int(l)]]["kps"][int(l)][1])
                   and np.array_equal(d["src_Twc"][d["src"][i]], M.kfs[A[int(l)]]["Twc"])
                   for i, l in enumerate(frame["lmid"]) if int(l) in A and int(l) in Bc)
        st, wpt, _ = T.keyframe(P, dict(d, is_stereo=np.zeros(frame["n"], np.uint8)))
        status, reason = {}, {}
        in_kf = set(int(l) for l in kf["lmid"])
        for i in range(frame["n"]):
            lm = int(frame["lmid"][i])
            status[lm] = int(st[i])
            if (st[i] & TRIED) and not (st[i] & OK):
                s = d["src"][i]
                reason[lm] = reject_reason(P, kf["Twc"], d["unpx"][i], d["bv"][i], d["src_Twc"][s], d["src_Tcw"][s], d["src_unpx"][i], d["src_bv"][i])
            if st[i] & OK:
                known[lm] = wpt[i].copy()
                M.update_point(lm)
            if st[i] & REMOVE_OBS:
                M.remove_obs(lm, kf["id"])
        gone = [lm for lm, s in status.items() if s & REMOVE_OBS]
        keep = np.array([int(l) not in gone for l in kf["lmid"]], bool)
        kf.update(lmid=kf["lmid"][keep], unpx=kf["unpx"][keep], bv=kf["bv"][keep])
        log.append(dict(k=k, tag=tag, a=A, b=Bc, same_src=same, status=status, reason=reason,
                        n_not_in_kf=sum(int(l) not in in_kf for l in frame["lmid"]), n_3d=int(frame["is3d"].sum()),
                        rows=[int(v) for v in tb.row_kfid], anchors={int(l): int(v) for l, v in zip(tb.lmid, tb.kfid)}))

    for k in range(N_KF):
        if k == 2:                                                         # local BA moved keyframe 0
            poses[0][:3] += np.array([0.004, -0.003, 0.002])
            M.kfs[kfid_of(0, b)]["Twc"] = poses[0].copy()
            tb.set_poses([(kfid_of(0, b), poses[0])])
        if k == 4:                                                         # the map culls keyframe 1; the caller re-anchors
            M.cull(kfid_of(1, b))
            tb = AnchorTable.from_map(M, tb.lmid)
        frame = frame_for(item, k, known)
        kf = keyframe_of(S, frame, kfid_of(k, b), poses[k])
        M.add_keyframe(kf["id"], kf["Twc"], kf["lmid"], kf["unpx"], kf["bv"], frame["is3d"][np.argsort(frame["lmid"], kind="stable")])
        call(k, kf, frame, "kf%d" % k)
        if k == 1:                                                         # a second call on the same keyframe
            call(k, kf, frame_for(item, k, known), "kf1_again")
    return log
