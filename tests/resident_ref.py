"""The resident frame (scope row f21) as what it replaces: a frame per item KEPT ON THE HOST and rebuilt by the caller between the
existing calls.
   apply_ops    the numpy specification of ov2_btracker_update_frame: what the map did to a frame, as (lmid, op, xyz) ops
   Route        the resident cycle on existing calls only -- trackmono_ref.route on arrays staged from the host frames, then
                trackmono_ref.frame_after to build the next frame (the tracked px of the kept slots, their lmid / is3d / wpt
                carried along, in slot order); createkf_ref.route for keyframes (a CREATED item's frame becomes the call's frame, the
                new points without a 3-D point); apply_ops for the map's updates.
A frame is dict(n, px (n, 2) float32, lmid (n,) int32, is3d (n,) uint8, wpt (n, 3) float64).  The GPU test holds the resident calls to
Route byte for byte."""
import numpy as np

from ov2slam_amd import _lib as L
from tests import createkf_ref, trackmono_ref

RESULT_KEYS = ("n_before", "n_after", "n_set", "n_unset", "n_removed", "n_missing")


def empty_frame():
    return dict(n=0, px=np.zeros((0, 2), np.float32), lmid=np.zeros(0, np.int32), is3d=np.zeros(0, np.uint8), wpt=np.zeros((0, 3), np.float64))


def make_frame(px, lmid, is3d, wpt):
    px = np.array(px, np.float32).reshape(-1, 2)
    return dict(n=len(px), px=px, lmid=np.array(lmid, np.int32).reshape(-1), is3d=(np.array(is3d).reshape(-1) != 0).astype(np.uint8),
                wpt=np.array(wpt, np.float64).reshape(-1, 3))


def apply_ops(frame, ops):
    """-> (the frame after the ops, the record).  ops: (lmid, op, xyz) with an lmid at most once.  SET_POINT: wpt = xyz, is3d = 1;
    UNSET_POINT: is3d = 0, wpt stays; REMOVE: the slot leaves and the rest close up in slot order; an lmid the frame does not hold is
    counted and changes nothing."""
    ids = [int(o[0]) for o in ops]
    assert len(set(ids)) == len(ids), "an lmid repeated within one list"
    n = int(frame["n"])
    slot = {int(frame["lmid"][i]): i for i in range(n)}
    assert len(slot) == n, "a frame holds an lmid once"
    is3d, wpt, keep = frame["is3d"][:n].copy(), frame["wpt"][:n].copy(), np.ones(n, bool)
    rec = dict.fromkeys(RESULT_KEYS, 0)
    for lmid, op, xyz in ops:
        i = slot.get(int(lmid))
        if i is None:
            rec["n_missing"] += 1
        elif op == L.OV2_RES_SET_POINT:
            wpt[i], is3d[i] = np.asarray(xyz, np.float64), 1
            rec["n_set"] += 1
        elif op == L.OV2_RES_UNSET_POINT:
            is3d[i] = 0
            rec["n_unset"] += 1
        elif op == L.OV2_RES_REMOVE:
            keep[i] = False
            rec["n_removed"] += 1
        else:
            raise ValueError("unknown op %r" % (op,))
    out = dict(n=int(keep.sum()), px=frame["px"][:n][keep].copy(), lmid=frame["lmid"][:n][keep].copy(), is3d=is3d[keep], wpt=wpt[keep])
    rec.update(n_before=n, n_after=out["n"])
    return out, rec


def frame_bytes(f):
    """what two frames are compared on: n, px / lmid / is3d of the slots, wpt where is3d"""
    n = int(f["n"])
    d3 = np.asarray(f["is3d"][:n], np.uint8)
    return dict(n=n, px=np.ascontiguousarray(f["px"][:n], np.float32).tobytes(), lmid=np.ascontiguousarray(f["lmid"][:n], np.int32).tobytes(),
                is3d=d3.tobytes(), wpt=np.ascontiguousarray(np.asarray(f["wpt"][:n], np.float64)[d3 != 0]).tobytes())


class Route:
    """the host-kept frames of a lock-step batch and the mirrors of trackmono_ref, advanced through the existing calls"""

    def __init__(self, batch, n_max):
        self.batch, self.n_max = batch, n_max
        self.frames = [empty_frame() for _ in range(batch)]
        self.mir = trackmono_ref.mirrors(batch)

    def set_frame(self, b, frame):
        self.frames[b] = dict(frame, px=frame["px"].copy(), lmid=frame["lmid"].copy(), is3d=frame["is3d"].copy(), wpt=frame["wpt"].copy())

    def update(self, n_active, ops):
        recs = []
        for b in range(n_active):
            self.frames[b], r = apply_ops(self.frames[b], ops[b])
            recs.append(r)
        return recs

    def arrays(self, na):
        """the frames of items [0, na) in the slot layout the existing calls take"""
        B, nm = self.batch, self.n_max
        a = dict(px=np.zeros((B, nm, 2), np.float32), lmid=np.zeros((B, nm), np.int32), is3d=np.zeros((B, nm), np.uint8),
                 wpt=np.zeros((B, nm, 3), np.float64), n=np.zeros(na, np.int32))
        for b in range(na):
            f = self.frames[b]
            n = f["n"]
            a["px"][b, :n], a["lmid"][b, :n], a["is3d"][b, :n], a["wpt"][b, :n], a["n"][b] = f["px"], f["lmid"], f["is3d"], f["wpt"], n
        return a

    def step(self, ctx, trk, imgs, params, epi_params, p3p_req, seed, nbkfs, epi_seed, time, frame_id, localba_is_on=None, doepipolar=True,
             dop3p=False, n_rows=0):
        """trackmono_ref.route on the host frames, then the next frames by frame_after -> what trackMonoResident returns"""
        na = len(imgs)
        first = self.mir["frames"] == 0
        a = self.arrays(na)
        out, st, rule, epis, poses, monos = trackmono_ref.route(ctx, trk, self.mir, imgs, a["px"], a["wpt"], a["is3d"], a["n"], params, epi_params,
                                                                p3p_req, seed, a["lmid"], nbkfs, epi_seed, time, frame_id,
                                                                localba_is_on=localba_is_on, doepipolar=doepipolar, dop3p=dop3p, n_rows=n_rows)
        frames = []
        tracked = not first and int(a["n"].sum()) > 0                       # else nothing ran: every frame stays
        for b in range(na):
            f = self.frames[b]
            if tracked:
                s = trackmono_ref.frame_after(st[b], f["n"], None if epis is None else epis[b], poses[b])
                self.frames[b] = dict(n=len(s), px=np.ascontiguousarray(out[b, s]), lmid=f["lmid"][s], is3d=f["is3d"][s], wpt=f["wpt"][s])
            frames.append(dict(n_before=int(f["n"]), n_after=int(self.frames[b]["n"])))
        return out, st, rule, epis, poses, monos, frames

    def create_keyframe(self, ctx, trk, cal, n_active, make_kf, nlmid, nkfid, time, params, state, out=None):
        """createkf_ref.route on the host frames with the mirrors' poses; a CREATED item's frame and the mirrors' keyframe follow"""
        a = self.arrays(n_active)
        Twc = self.mir["poses"][:n_active].copy()
        recs, out = createkf_ref.route(ctx, trk, cal, n_active, a["px"], a["lmid"], a["is3d"], a["n"], make_kf, nlmid, nkfid, time, params, state,
                                       Twc=Twc, out=out)
        for b, r in enumerate(recs):
            if r["action"] != L.OV2_CKF_CREATED:
                continue
            m0, m = r["n_prev"], r["n_kf"]
            f = self.frames[b]
            self.frames[b] = dict(n=m, px=out["px"][b, :m].copy(), lmid=out["lmid"][b, :m].copy(),
                                  is3d=np.concatenate([f["is3d"][:m0], np.zeros(m - m0, np.uint8)]),
                                  wpt=np.concatenate([f["wpt"][:m0], np.zeros((m - m0, 3))]))
            o = np.argsort(out["lmid"][b, :m], kind="stable")
            self.mir["keyframes"][b] = dict(lmid=out["lmid"][b, :m][o].copy(), unpx=out["unpx"][b, :m][o].copy(), bv=out["bv"][b, :m][o].copy(),
                                            Twc=Twc[b].copy())
            self.mir["info"][b] = (int(nkfid[b]), float(time[b]), r["nb3dkps"])
        return recs, out
