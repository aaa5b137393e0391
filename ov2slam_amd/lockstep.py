"""LockstepTracker: `batch` camera streams in lock-step on top of ov2_btracker_* (include/ov2slam_hip.h, csrc/trackb.hip).

Every lock-step call family of the C ABI (track_frame ... temporal_keyframe, mono_init) comes as three entry points -- the whole call, _begin
and _end --, and the argument list of the whole call is _begin's followed by _end's.  The binding has one path for all of them:

    _marshal_<family>(public arguments) -> _Call      what _begin takes, and every array and struct those arguments point at
    _Results(tracker, family, call)                   what _end takes: the buffers it fills, and finish() -> the Python return value
    _whole / _begin / _end                            the three drivers every public method goes through

The tracker holds at most one _Call, the open one (`_open`), as the library holds one open call; it is installed only after the
library has accepted the _begin.  A new lock-step call is one _marshal_ function, one entry in a _Results table and three
one-line methods.  _Call and _Results are also the seam for tests that call the ABI directly: marshal, change a struct field
(`call.inputs.Twc_h = None`), and pass `*call.args` on."""
import ctypes as C

import numpy as np

from . import _lib as L
from .frontend import _PyrView, _ptr, _roi_arg


class _Call:
    """One marshalled lock-step call.  family: the stem of the entry points (ov2_btracker_<family>[_begin]); na: n_active; args: the
    arguments of _begin after the handle; params / inputs: the structs args points at (None for a family without them), to be
    changed in place before the call; keep: by name, every array args or the structs point at -- they live as long as the record
    does, which is until _end for an open call; nn: the per-item keypoint counts the result side cuts by (None: the frames are
    resident, the step reports them); epi: whether _end is to fill epipolar results."""

    def __init__(self, family, na, args, nn=None, params=None, inputs=None, **keep):
        self.family, self.na, self.args, self.nn, self.params, self.inputs, self.keep, self.epi = family, na, args, nn, params, inputs, keep, True

    def extend(self, family, params, inputs, **keep):
        """the call of the family one above: the same arguments, then its two structs"""
        self.family, self.params, self.inputs = family, params, inputs
        self.args += (C.byref(params), C.byref(inputs))
        self.keep.update(keep)
        return self


def _scatter(shapes, lead, out):
    """the arrays a keyframe _end scatters into (the caller's, so that untouched slots stay what they were, or fresh zeros)"""
    o = {}
    for k, (tail, dt) in shapes.items():
        a, shape = None if out is None else out.get(k), lead + tail
        if a is None:
            a = np.zeros(shape, dt)
        elif a.dtype != dt or a.shape != shape or not a.flags.c_contiguous:
            raise ValueError("out[%r] must be a contiguous %s array of shape %r" % (k, np.dtype(dt).name, shape))
        o[k] = a
    return o


class _Results:
    """The result side of one call of `family` for the marshalled `call` (None: nothing is open, the buffers are sized for no item
    and the library refuses).  args: the arguments of _end after the handle; finish(): the Python return value.  A step family has
    out / st / p3p and, by STEP, the per-item E (epipolar, with bufs), R (pose, with removed), M (mono) and F (resident frame)
    results; a keyframe family has the per-item records R and the dict `out` of slot-layout arrays."""

    STEP = {"track_frame": "", "track_frame_map": "", "track_frame_pose": "R", "track_frame_epi_pose": "ER", "track_mono": "ERM",
            "track_mono_resident": "ERMF"}
    # family -> (per-item result struct, the record's keys, {name: (shape after (batch, n_max), dtype)} in the order of _end's arguments)
    KEYFRAME = {
        "create_keyframe": (L.CreateKeyframeResult, ("action", "n_prev", "noccupcells", "nb2detect", "n_new", "n_kf", "nb3dkps"),
                            dict(px=((2,), np.float32), lmid=((), np.int32), unpx=((2,), np.float32), bv=((3,), np.float64),
                                 desc=((L.OV2_BRIEF_BYTES,), np.uint8), valid=((), np.uint8), color=((), np.uint8))),
        "stereo_keyframe": (L.StereoKeyframeResult, tuple(k for k, _ in L.StereoKeyframeResult._fields_),
                            dict(right_px=((2,), np.float32), stereo_ok=((), np.uint8), tri_status=((), np.uint8), wpt=((3,), np.float64),
                                 invdepth=((), np.float64))),
        "temporal_keyframe": (L.TemporalKeyframeResult, tuple(k for k, _ in L.TemporalKeyframeResult._fields_),
                              dict(tri_status=((), np.uint8), wpt=((3,), np.float64), invdepth=((), np.float64), src_kfid=((), np.int32))),
        # (keys None: the record holds floats and arrays, keyframe._mono_init_record reads it)
        "mono_init": (L.MonoInitResult, None, dict(removed=((), np.uint8))),
    }

    def __init__(self, trk, family, call, out=None):
        self.family = family
        self.na = na = call.na if call is not None else 0
        self.nn = call.nn if call is not None and call.nn is not None else np.zeros(na, np.int32)
        rows, slots = max(1, na), (trk.batch, trk.n_max)
        if family in self.KEYFRAME:
            rtype, self.keys, shapes = self.KEYFRAME[family]
            self.R, self.out = (rtype * rows)(), _scatter(shapes, slots, out)
            self.args = (self.R,) + tuple(_ptr(self.out[k]) for k in shapes)
            return
        self.parts = self.STEP[family]
        self.out, self.st, self.p3p = np.zeros(slots + (2,), np.float32), np.zeros(slots, np.uint8), np.zeros(na, np.int32)
        self.args = (_ptr(self.out), _ptr(self.st), _ptr(self.p3p))
        if "E" in self.parts:
            self.E, self.epi = (L.EpifilterResult * rows)(), call.epi if call is not None else True
            self.bufs = dict(removed=np.zeros((rows, trk.n_max), np.uint8), pair_cur=np.zeros((rows, trk.n_max), np.int32),
                             err=np.zeros((rows, trk.n_max), np.float32))
            for b in range(na):
                self.E[b].removed = self.bufs["removed"][b].ctypes.data_as(C.POINTER(C.c_uint8))
                self.E[b].pair_cur = self.bufs["pair_cur"][b].ctypes.data_as(C.POINTER(C.c_int))
                self.E[b].err = self.bufs["err"][b].ctypes.data_as(C.POINTER(C.c_float))
            self.args += (self.E if self.epi else None,)
        if "R" in self.parts:
            self.R, self.removed = (L.PoseResult * rows)(), np.zeros((rows, trk.n_max), np.uint8)
            for b in range(na):
                self.R[b].removed = self.removed[b].ctypes.data_as(C.POINTER(C.c_uint8))
            self.args += (self.R,)
        if "M" in self.parts:
            self.M = (L.TrackMonoResult * rows)()
            self.args += (self.M,)
        if "F" in self.parts:
            self.F = (L.ResidentStepResult * rows)()
            self.args += (self.F,)

    def finish(self):
        from . import keyframe as _kf
        from . import motion as _motion
        from . import pose as _pose
        na, nn = self.na, self.nn
        if self.family in self.KEYFRAME:
            if self.keys is None:
                return [_kf._mono_init_record(self.R[b]) for b in range(na)], self.out
            return [{k: int(getattr(self.R[b], k)) for k in self.keys} for b in range(na)], self.out
        res = (self.out, self.st, self.p3p.astype(bool))
        if "F" in self.parts:
            nn = np.array([self.F[b].n_before for b in range(na)], np.int32)
        if "E" in self.parts:
            E, bufs = self.E, self.bufs
            res += ([_kf._epifilter_dict(E[b], dict(removed=bufs["removed"][b, :int(nn[b])], pair_cur=bufs["pair_cur"][b],
                                                    err=bufs["err"][b, :int(nn[b])])) for b in range(na)] if self.epi else None,)
        if "R" in self.parts:
            res += ([_pose._pose_finish(self.R[b], dict(unpx=self.removed[b, :int(nn[b])], removed=self.removed[b])) for b in range(na)],)
        if "M" in self.parts:
            M = self.M
            res += ([dict(Twc_pred=np.array(M[b].Twc_pred[:], np.float64), resynced=int(M[b].resynced), state=_motion._state_dict(M[b].state),
                          kf=_kf._decision_dict(M[b].kf)) for b in range(na)],)
        if "F" in self.parts:
            res += ([dict(n_before=int(self.F[b].n_before), n_after=int(self.F[b].n_after)) for b in range(na)],)
        return res


class LockstepTracker:
    """`batch` camera streams in lock-step (ov2_btracker_*, csrc/trackb.hip): the offline batch-of-sequences form of
    VisualFrontEndTracker.  Every call advances items [0, n_active) by one frame with ONE enqueue over all of them; results per
    item are bit-identical to a VisualFrontEndTracker fed the same frames and keypoints.  Point arrays are (batch, n_max, 2) with
    n[b] valid rows per item."""

    def __init__(self, ctx, batch, w, h, nklt_win_size=9, nklt_pyr_lvl=3, nmax_iter=30, fmax_px_precision=0.01, nklt_err=30.0,
                 fmax_fbklt_dist=0.5, use_clahe=True, fclahe_val=3.0, nbmaxkps=512, prior_pyr_lvl=1):
        self.ctx, self.lib = ctx, ctx.lib
        self.batch, self.w, self.h, self.win, self.n_max = int(batch), int(w), int(h), int(nklt_win_size), int(nbmaxkps)
        self._open = None                             # the _Call between its _begin and its _end (the library holds one, too)
        self._rmap = None                             # (keeps the RectifyMap of setRectification alive)
        self._n_src_max = L.OV2_TKF_MAX_ROWS          # rows of an item's anchor table, once reserveAnchors / temporalKeyframe fixed them
        cfg = L.TrackerConfig(self.w, self.h, self.win, int(nklt_pyr_lvl), int(prior_pyr_lvl), int(nmax_iter),
                              float(np.float32(fmax_px_precision)), float(nklt_err), float(fmax_fbklt_dist),
                              int(bool(use_clahe)), float(fclahe_val), self.w // 50, self.h // 50, self.n_max, 0)
        ht = C.c_void_p()
        L.check(self.lib.ov2_btracker_create(ctx.h, C.byref(cfg), self.batch, C.byref(ht)))
        self.h_trk = ht
        ctx._children.add(self)
        stride = C.c_int()
        self.image_buffers = []                       # [which][item] -> numpy view of the pinned slot
        for which in range(3):
            row = []
            for b in range(self.batch):
                ptr = self.lib.ov2_btracker_image_buffer(ht, which, b, C.byref(stride))
                row.append(np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(self.h, stride.value)))
            self.image_buffers.append(row)
        self.stride = stride.value

    def setCalibration(self, calib):
        L.check(self.lib.ov2_btracker_set_calibration(self.h_trk, calib.model, _ptr(calib.K), _ptr(calib.D) if calib.D is not None else None,
                                                      0 if calib.D is None else len(calib.D), _ptr(calib.iK)))

    def setRectification(self, rmap):
        """rmap: RectifyMap or None: the frames of trackFrame / upload / prepare are RAW from now on (rectified in the same enqueue,
        before CLAHE).  Between steps only."""
        L.check(self.lib.ov2_btracker_set_rectification(self.h_trk, rmap.h_map if rmap is not None else None))
        self._rmap = rmap

    def upload(self, which, n_active):
        """start the H2D of staging set `which` (already filled through image_buffers[which]) on the copy stream"""
        L.check(self.lib.ov2_btracker_upload(self.h_trk, int(which), int(n_active)))

    def prepare(self, which, n_active):
        """preprocessImage of staging set `which` for the NEXT trackFrame, on the tracker's prep stream"""
        L.check(self.lib.ov2_btracker_prepare(self.h_trk, int(which), int(n_active)))

    # ---- the three drivers: every lock-step call below goes through them -----------------------------------------------------------
    def _whole(self, call, out=None):
        """the one-call entry (it checks the result buffers before it opens the step): _begin's arguments, then _end's"""
        res = _Results(self, call.family, call, out)
        L.check(getattr(self.lib, "ov2_btracker_" + call.family)(self.h_trk, *call.args, *res.args))
        return res.finish()

    def _begin(self, call):
        L.check(getattr(self.lib, "ov2_btracker_%s_begin" % call.family)(self.h_trk, *call.args))
        self._open = call                             # (only now: a refused _begin leaves the open call as it was)

    def _end(self, family, out=None):
        """finishes the open call as `family` finishes it; with nothing open, or a call of another kind, the library refuses"""
        res = _Results(self, family, self._open, out)
        L.check(getattr(self.lib, "ov2_btracker_%s_end" % family)(self.h_trk, *res.args))
        self._open = None
        return res.finish()

    # ---- marshalling: one function per family, each on top of the one below it ---------------------------------------------------------
    def _marshal_frames(self, family, imgs, klt_use_prior):
        """the frames of a step -> (n_active, pointer array, common row pitch, klt_use_prior); refuses a wrong shape or mixed pitches"""
        imgs = [im if im.dtype == np.uint8 and im.strides[1] == 1 else np.ascontiguousarray(im, np.uint8) for im in imgs]
        stride = imgs[0].strides[0]
        for im in imgs:
            if im.ndim != 2 or im.shape[0] != self.h or im.shape[1] < self.w or im.strides[0] != stride:
                raise ValueError("frames must be %d rows of >= %d bytes with one common row pitch" % (self.h, self.w))
        ptrs = (C.c_void_p * len(imgs))(*[im.ctypes.data for im in imgs])
        return _Call(family, len(imgs), (len(imgs), ptrs, stride, int(bool(klt_use_prior))), imgs=imgs, ptrs=ptrs)

    def _marshal_track_frame(self, imgs, kps, pri, hasprior, n, klt_use_prior=True):
        c = self._marshal_frames("track_frame", imgs, klt_use_prior)
        kps = np.ascontiguousarray(kps, np.float32).reshape(self.batch, self.n_max, 2)
        pri = np.ascontiguousarray(pri, np.float32).reshape(self.batch, self.n_max, 2)
        hp = None if hasprior is None else np.ascontiguousarray(hasprior, np.uint8).reshape(self.batch, self.n_max)
        c.nn = nn = np.ascontiguousarray(n, np.int32)
        if len(nn) != c.na:
            raise ValueError("one keypoint count per active item")
        c.args = c.args[:3] + (_ptr(kps), _ptr(pri), _ptr(hp), _ptr(nn)) + c.args[3:]
        c.keep.update(kps=kps, pri=pri, hasprior=hp, n=nn)                        # (kps / hasprior are re-read by _end)
        return c

    def _marshal_track_frame_map(self, imgs, kps, wpt, is3d, Tcw, n, klt_use_prior=True):
        c = self._marshal_frames("track_frame_map", imgs, klt_use_prior)
        kps = np.ascontiguousarray(kps, np.float32).reshape(self.batch, self.n_max, 2)
        wpt = np.ascontiguousarray(wpt, np.float64).reshape(self.batch, self.n_max, 3)
        is3d = np.ascontiguousarray(is3d, np.uint8).reshape(self.batch, self.n_max)
        Tcw = np.ascontiguousarray(Tcw, np.float64).reshape(-1, 7)
        c.nn = nn = np.ascontiguousarray(n, np.int32)
        if len(nn) != c.na or len(Tcw) < c.na:
            raise ValueError("one keypoint count and one predicted pose per active item")
        c.args = c.args[:3] + (_ptr(kps), _ptr(wpt), _ptr(is3d), _ptr(Tcw), _ptr(nn)) + c.args[3:]
        c.keep.update(kps=kps, wpt=wpt, is3d=is3d, Tcw=Tcw, n=nn)                 # (kps is re-read by _end)
        return c

    def _pose_structs(self, na, params, Twc, p3p_req, seed, scale, dop3p, n_rows):
        """-> (ov2_frame_pose_params, ov2_frame_pose_input, the arrays the input points at)"""
        from . import pose as _pose
        fp = L.FramePoseParams()
        fp.pose, fp.dop3p, fp.n_rows = _pose._as_pose_params(params), int(bool(dop3p)), int(n_rows)
        Twc = np.ascontiguousarray(Twc, np.float64).reshape(-1, 7)
        req = np.ascontiguousarray(p3p_req, np.uint8).reshape(-1)
        seed = np.ascontiguousarray(seed, np.uint64).reshape(-1)
        sc = None if scale is None else np.ascontiguousarray(scale, np.int32).reshape(self.batch, self.n_max)
        if len(Twc) < na or len(req) < na or len(seed) < na:
            raise ValueError("one pose, one p3p request and one seed per active item")
        fi = L.FramePoseInput()
        fi.Twc_h = Twc.ctypes.data_as(C.POINTER(C.c_double))
        fi.scale_h = None if sc is None else sc.ctypes.data_as(C.POINTER(C.c_int))
        fi.p3p_req_h = req.ctypes.data_as(C.POINTER(C.c_uint8))
        fi.seed_h = seed.ctypes.data_as(C.POINTER(C.c_ulonglong))
        return fp, fi, dict(Twc=Twc, p3p_req=req, seed=seed, scale=sc)

    def _epi_structs(self, na, params, epi_params, Twc, p3p_req, seed, lmid, nbkfs, epi_seed, scale, dop3p, n_rows):
        """-> (ov2_frame_epi_pose_params, ov2_frame_epi_pose_input, the arrays the input points at)"""
        from . import keyframe as _kf
        fp, fi, keep = self._pose_structs(na, params, Twc, p3p_req, seed, scale, dop3p, n_rows)
        ep = L.FrameEpiPoseParams()
        ep.pose, ep.epi = fp, _kf._as_epifilter_params(epi_params)
        lm = np.ascontiguousarray(lmid, np.int32).reshape(self.batch, self.n_max)
        nk = np.ascontiguousarray(nbkfs, np.int32).reshape(-1)
        es = np.ascontiguousarray(epi_seed, np.uint64).reshape(-1)
        if len(nk) < na or len(es) < na:
            raise ValueError("one nbkfs and one epipolar seed per active item")
        ei = L.FrameEpiPoseInput()
        ei.pose = fi
        ei.lmid_h = lm.ctypes.data_as(C.POINTER(C.c_int))
        ei.nbkfs_h = nk.ctypes.data_as(C.POINTER(C.c_int))
        ei.epi_seed_h = es.ctypes.data_as(C.POINTER(C.c_ulonglong))
        return ep, ei, dict(keep, lmid=lm, nbkfs=nk, epi_seed=es)

    def _mono_structs(self, na, params, epi_params, p3p_req, seed, lmid, nbkfs, epi_seed, time, frame_id, localba_is_on, doepipolar, scale,
                      dop3p, n_rows):
        """-> (ov2_track_mono_params, ov2_track_mono_input, the arrays the input points at); lmid None: the frames are resident"""
        ep, ei, keep = self._epi_structs(na, params, epi_params, np.zeros((max(1, na), 7)), p3p_req, seed,
                                         np.zeros((self.batch, self.n_max), np.int32) if lmid is None else lmid,
                                         np.zeros(self.batch, np.int32) if nbkfs is None else nbkfs,
                                         np.zeros(self.batch, np.uint64) if epi_seed is None else epi_seed, scale, dop3p, n_rows)
        ei.pose.Twc_h = None                                                      # the pose is resident
        if lmid is None:
            ei.lmid_h = None                                                      # ... and so is the frame (trackMonoResident)
        mp, mi = L.TrackMonoParams(), L.TrackMonoInput()
        mp.step, mp.doepipolar = ep, int(bool(doepipolar))
        tm = np.ascontiguousarray(time, np.float64).reshape(-1)
        fid = np.ascontiguousarray(frame_id, np.int32).reshape(-1)
        ba = None if localba_is_on is None else np.ascontiguousarray(localba_is_on, np.uint8).reshape(-1)
        if len(tm) < na or len(fid) < na or (ba is not None and len(ba) < na):
            raise ValueError("one time, one frame id and one local-BA flag per active item")
        mi.step = ei
        mi.time_h = tm.ctypes.data_as(C.POINTER(C.c_double))
        mi.frame_id_h = fid.ctypes.data_as(C.POINTER(C.c_int))
        mi.localba_is_on_h = None if ba is None else ba.ctypes.data_as(C.POINTER(C.c_uint8))
        return mp, mi, dict(keep, time=tm, frame_id=fid, localba_is_on=ba)

    def _marshal_track_frame_pose(self, imgs, kps, wpt, is3d, Tcw, n, params, Twc, p3p_req, seed, scale=None, dop3p=False, n_rows=0,
                                  klt_use_prior=True):
        c = self._marshal_track_frame_map(imgs, kps, wpt, is3d, Tcw, n, klt_use_prior)
        fp, fi, keep = self._pose_structs(c.na, params, Twc, p3p_req, seed, scale, dop3p, n_rows)
        return c.extend("track_frame_pose", fp, fi, **keep)

    def _marshal_track_frame_epi_pose(self, imgs, kps, wpt, is3d, Tcw, n, params, epi_params, Twc, p3p_req, seed, lmid, nbkfs, epi_seed,
                                      scale=None, dop3p=False, n_rows=0, klt_use_prior=True):
        c = self._marshal_track_frame_map(imgs, kps, wpt, is3d, Tcw, n, klt_use_prior)
        ep, ei, keep = self._epi_structs(c.na, params, epi_params, Twc, p3p_req, seed, lmid, nbkfs, epi_seed, scale, dop3p, n_rows)
        return c.extend("track_frame_epi_pose", ep, ei, **keep)

    def _marshal_track_mono(self, imgs, kps, wpt, is3d, n, params, epi_params, p3p_req, seed, lmid, nbkfs, epi_seed, time, frame_id,
                            localba_is_on=None, doepipolar=True, scale=None, dop3p=False, n_rows=0, klt_use_prior=True):
        c = self._marshal_track_frame_map(imgs, kps, wpt, is3d, np.zeros((max(1, len(imgs)), 7)), n, klt_use_prior)
        c.args = c.args[:6] + c.args[7:]                                          # (no Tcw: the pose is resident)
        mp, mi, keep = self._mono_structs(c.na, params, epi_params, p3p_req, seed, lmid, nbkfs, epi_seed, time, frame_id, localba_is_on,
                                          doepipolar, scale, dop3p, n_rows)
        c.epi = bool(doepipolar)
        return c.extend("track_mono", mp, mi, **keep)

    def _marshal_track_mono_resident(self, imgs, params, epi_params, p3p_req, seed, nbkfs, epi_seed, time, frame_id, localba_is_on=None,
                                     doepipolar=True, dop3p=False, n_rows=0, klt_use_prior=True):
        c = self._marshal_frames("track_mono_resident", imgs, klt_use_prior)
        mp, mi, keep = self._mono_structs(c.na, params, epi_params, p3p_req, seed, None, nbkfs, epi_seed, time, frame_id, localba_is_on,
                                          doepipolar, None, dop3p, n_rows)
        c.epi = bool(doepipolar)
        return c.extend("track_mono_resident", mp, mi, **keep)

    def _marshal_create_keyframe(self, n_active, px, lmid, is3d, n, make_kf, nlmid, nkfid, time, params, state, Twc=None):
        na = int(n_active)
        cp = L.CreateKeyframeParams()
        cp.ncellsize, cp.nbwcells, cp.nbhcells, cp.nbmaxkps = (int(params[k]) for k in ("ncellsize", "nbwcells", "nbhcells", "nbmaxkps"))
        det = params.get("detector", "singlescale")
        cp.detector = {"singlescale": L.OV2_CKF_DET_SINGLESCALE, "gridfast": L.OV2_CKF_DET_GRID_FAST, "gftt": L.OV2_CKF_DET_GFTT}.get(det, det)
        cp.det_cell = int(params["det_cell"])
        cp.roi = (C.c_int * 4)(*[int(v) for v in params.get("roi", (0, 0, self.w, self.h))])
        cp.mask_mode = int(params.get("mask_mode", L.OV2_MASK_AS_EXECUTED))
        cp.do_subpix, cp.use_brief = int(bool(params.get("do_subpix", True))), int(bool(params.get("use_brief", True)))
        resident = px is None                                                     # the frame is the resident one
        if resident and not (lmid is None and is3d is None and n is None):
            raise ValueError("px None means the resident frame: lmid, is3d and n must be None too")
        px = None if resident else np.ascontiguousarray(px, np.float32).reshape(self.batch, self.n_max, 2)
        lm = None if resident else np.ascontiguousarray(lmid, np.int32).reshape(self.batch, self.n_max)
        d3 = None if resident else np.ascontiguousarray(is3d, np.uint8).reshape(self.batch, self.n_max)
        nn = np.zeros(na, np.int32) if resident else np.ascontiguousarray(n, np.int32).reshape(-1)
        mk = np.ascontiguousarray(make_kf, np.uint8).reshape(-1)
        nl = np.ascontiguousarray(nlmid, np.int32).reshape(-1)
        ki = np.ascontiguousarray(nkfid, np.int32).reshape(-1)
        tm = np.ascontiguousarray(time, np.float64).reshape(-1)
        if min(len(nn), len(mk), len(nl), len(ki), len(tm)) < na:
            raise ValueError("one count, flag, nlmid, keyframe id and time per active item")
        T = None if Twc is None else np.ascontiguousarray(Twc, np.float64).reshape(-1, 7)
        if T is not None and len(T) < na:
            raise ValueError("one pose per active item")
        fast = cp.detector == L.OV2_CKF_DET_GRID_FAST
        st = np.ascontiguousarray(state, np.int32 if fast else np.float64)
        assert st is state or np.shares_memory(st, state), "state must be a contiguous int32 (FAST) / float64 (single scale) array (updated in place)"
        if len(st) < na:
            raise ValueError("one adaptive state per active item")
        ci = L.CreateKeyframeInput()
        ci.px_h = None if resident else px.ctypes.data_as(C.POINTER(C.c_float))
        ci.lmid_h = None if resident else lm.ctypes.data_as(C.POINTER(C.c_int))
        ci.is3d_h = None if resident else d3.ctypes.data_as(C.POINTER(C.c_uint8))
        ci.n_h = None if resident else nn.ctypes.data_as(C.POINTER(C.c_int))
        ci.make_kf_h = mk.ctypes.data_as(C.POINTER(C.c_uint8))
        ci.nlmid_h = nl.ctypes.data_as(C.POINTER(C.c_int))
        ci.nkfid_h = ki.ctypes.data_as(C.POINTER(C.c_int))
        ci.time_h = tm.ctypes.data_as(C.POINTER(C.c_double))
        ci.Twc_h = None if T is None else T.ctypes.data_as(C.POINTER(C.c_double))
        ci.quality_inout = None if fast else st.ctypes.data_as(C.POINTER(C.c_double))
        ci.fast_th_inout = st.ctypes.data_as(C.POINTER(C.c_int)) if fast else None
        return _Call("create_keyframe", na, (na,), px=px, lmid=lm, is3d=d3, n=nn, make_kf=mk, nlmid=nl, nkfid=ki, time=tm, Twc=T,
                     state=st).extend("create_keyframe", cp, ci)                  # (state is updated by _end)

    def _marshal_stereo_keyframe(self, n_active, right_pyr, do, params):
        c = self._marshal_temporal_keyframe(n_active, do, params)
        c.family, c.args = "stereo_keyframe", c.args[:2] + (right_pyr.h_pyr,) + c.args[2:]
        c.keep.update(right_pyr=right_pyr)
        return c

    def _marshal_temporal_keyframe(self, n_active, do, params):
        na = int(n_active)
        d = np.ascontiguousarray(do, np.uint8).reshape(-1)
        if len(d) < na:
            raise ValueError("one flag per active item")
        return _Call("temporal_keyframe", na, (na, C.byref(params), _ptr(d)), params=params, do=d)

    def _marshal_mono_init(self, n_active, do, seed, params):
        from . import keyframe as _kf
        c = self._marshal_temporal_keyframe(n_active, do, _kf._as_mono_init_params(params))
        sd = np.ascontiguousarray(seed, np.uint64).reshape(-1)
        if len(sd) < c.na:
            raise ValueError("one seed per active item")
        c.family, c.args = "mono_init", c.args + (_ptr(sd),)
        c.keep.update(seed=sd)
        return c

    # ---- the lock-step calls ------------------------------------------------------------------------------------------------------------
    def trackFrame(self, imgs, kps, pri, hasprior, n, klt_use_prior=True):
        """imgs: list of n_active (h, >=w) uint8 arrays of one row pitch (or pinned slots of one staging set); kps / pri:
        (batch, n_max, 2) float32; hasprior: (batch, n_max) uint8 or None; n: per-item counts (len n_active).
        -> (out (batch, n_max, 2), status bits (batch, n_max), p3p_req (n_active,) bool)"""
        return self._whole(self._marshal_track_frame(imgs, kps, pri, hasprior, n, klt_use_prior))

    def trackFrameBegin(self, imgs, kps, pri, hasprior, n, klt_use_prior=True):
        """first half of trackFrame: enqueue the step and return (upload / prepare of the frames to come go between the halves)"""
        self._begin(self._marshal_track_frame(imgs, kps, pri, hasprior, n, klt_use_prior))

    def trackFrameEnd(self):
        """second half: wait, results, p3p rule -> (out, status bits, p3p_req) as trackFrame"""
        return self._end("track_frame")

    def trackFrameMap(self, imgs, kps, wpt, is3d, Tcw, n, klt_use_prior=True):
        """trackFrame with the priors derived on the device (ov2_btracker_track_frame_map): wpt (batch, n_max, 3) float64 map points,
        is3d (batch, n_max) uint8, Tcw (>= n_active, 7) the predicted poses [t q], already inverted.  Needs setCalibration.
        -> (out, status bits, p3p_req) as trackFrame; lastPriors returns the priors that were used."""
        return self._whole(self._marshal_track_frame_map(imgs, kps, wpt, is3d, Tcw, n, klt_use_prior))

    track_frame_map = trackFrameMap

    def trackFrameMapBegin(self, imgs, kps, wpt, is3d, Tcw, n, klt_use_prior=True):
        """first half of trackFrameMap; trackFrameEnd finishes it"""
        self._begin(self._marshal_track_frame_map(imgs, kps, wpt, is3d, Tcw, n, klt_use_prior))

    def trackFramePose(self, imgs, kps, wpt, is3d, Tcw, n, params, Twc, p3p_req, seed, scale=None, dop3p=False, n_rows=0,
                       klt_use_prior=True):
        """trackFrameMap and the per-frame pose in one enqueue and one synchronisation (ov2_btracker_track_frame_pose).  params: as
        pose.compute_pose takes them; Twc (>= n_active, 7): the predicted poses NOT inverted (Tcw: the same, inverted); p3p_req, seed:
        one per item; scale (batch, n_max) int or None; dop3p, n_rows: SlamParams::dop3p_ and the rows of the table drawn for an item
        that searches.  -> (out, status bits, p3p_req, poses): poses[b] as pose.compute_pose returns it, with removed (n[b],) IN SLOT
        SPACE."""
        return self._whole(self._marshal_track_frame_pose(imgs, kps, wpt, is3d, Tcw, n, params, Twc, p3p_req, seed, scale, dop3p, n_rows,
                                                          klt_use_prior))

    def trackFramePoseBegin(self, imgs, kps, wpt, is3d, Tcw, n, params, Twc, p3p_req, seed, scale=None, dop3p=False, n_rows=0,
                            klt_use_prior=True):
        """first half of trackFramePose; trackFramePoseEnd finishes it (trackFrameEnd finishes the tracking half and drops the pose)"""
        self._begin(self._marshal_track_frame_pose(imgs, kps, wpt, is3d, Tcw, n, params, Twc, p3p_req, seed, scale, dop3p, n_rows,
                                                   klt_use_prior))

    def trackFramePoseEnd(self):
        """second half of trackFramePose -> (out, status bits, p3p_req, poses)"""
        return self._end("track_frame_pose")

    def lastPoseInputs(self, item):
        """what the last pose step fed the chain for `item` -> (m, slots (m,) int32, samples (rows used, 4) int32)"""
        m, rows = C.c_int(), C.c_int()
        slot = np.zeros(self.n_max, np.int32)
        tab = np.zeros((L.OV2_P3P_MAX_ROWS, 4), np.int32)                         # (room for the most rows a finished step can have drawn)
        L.check(self.lib.ov2_btracker_last_pose_inputs(self.h_trk, int(item), C.byref(m), slot.ctypes.data_as(C.POINTER(C.c_int)),
                                                       tab.ctypes.data_as(C.POINTER(C.c_int)), C.byref(rows)))
        return m.value, slot[:m.value].copy(), tab[:rows.value].copy()

    def setKeyframe(self, item, kf_lmid, kf_unpx, kf_bv, kf_Twc):
        """the keyframe item `item` is filtered against from now on (ov2_btracker_set_keyframe): kf_lmid (m,) strictly ascending,
        kf_unpx (m, 2), kf_bv (m, 3), kf_Twc (7,); it stays on the device until it is replaced.  m == 0 takes it away.  Between
        steps only."""
        lm = np.ascontiguousarray(kf_lmid, np.int32).reshape(-1)
        un = np.ascontiguousarray(kf_unpx, np.float32).reshape(-1, 2)
        bv = np.ascontiguousarray(kf_bv, np.float64).reshape(-1, 3)
        if len(un) != len(lm) or len(bv) != len(lm):
            raise ValueError("one unpx and one bearing per keyframe id")
        T = None if kf_Twc is None else np.ascontiguousarray(kf_Twc, np.float64).reshape(7)
        L.check(self.lib.ov2_btracker_set_keyframe(self.h_trk, int(item), len(lm), _ptr(lm), _ptr(un), _ptr(bv), _ptr(T)))

    def trackFrameEpiPose(self, imgs, kps, wpt, is3d, Tcw, n, params, epi_params, Twc, p3p_req, seed, lmid, nbkfs, epi_seed,
                          scale=None, dop3p=False, n_rows=0, klt_use_prior=True):
        """trackFrameMap, epipolar2d2dFiltering against the resident keyframes (setKeyframe) and the per-frame pose in one enqueue and
        one synchronisation (ov2_btracker_track_frame_epi_pose): trackMono's per-frame sequence with doepipolar_ == 1.  As
        trackFramePose, plus epi_params (as keyframe.epipolar_filter takes them; boptimize False), lmid (batch, n_max) int32, nbkfs
        and epi_seed one per item.  -> (out, status bits, p3p_req, epis, poses): epis[b] as keyframe.epipolar_filter returns it with
        removed / err (n[b],) and pair_cur (m,) IN SLOT SPACE; poses[b] as trackFramePose, on the frame after the filter."""
        return self._whole(self._marshal_track_frame_epi_pose(imgs, kps, wpt, is3d, Tcw, n, params, epi_params, Twc, p3p_req, seed, lmid, nbkfs,
                                                              epi_seed, scale, dop3p, n_rows, klt_use_prior))

    def trackFrameEpiPoseBegin(self, imgs, kps, wpt, is3d, Tcw, n, params, epi_params, Twc, p3p_req, seed, lmid, nbkfs, epi_seed,
                               scale=None, dop3p=False, n_rows=0, klt_use_prior=True):
        """first half of trackFrameEpiPose; trackFrameEpiPoseEnd finishes it (trackFrameEnd finishes the tracking half and drops both
        results)"""
        self._begin(self._marshal_track_frame_epi_pose(imgs, kps, wpt, is3d, Tcw, n, params, epi_params, Twc, p3p_req, seed, lmid, nbkfs,
                                                       epi_seed, scale, dop3p, n_rows, klt_use_prior))

    def trackFrameEpiPoseEnd(self):
        """second half of trackFrameEpiPose -> (out, status bits, p3p_req, epis, poses)"""
        return self._end("track_frame_epi_pose")

    def lastEpiInputs(self, item):
        """what the last epipolar step fed the filter for `item` -> (n_cur, slots (n_cur,) int32, m, samples (rows used, 8) int32)"""
        nc, m, rows = C.c_int(), C.c_int(), C.c_int()
        slot = np.zeros(self.n_max, np.int32)
        tab = np.zeros((L.OV2_EPI_MAX_ROWS, 8), np.int32)                         # (room for the most rows a finished step can have drawn)
        L.check(self.lib.ov2_btracker_last_epi_inputs(self.h_trk, int(item), C.byref(nc), slot.ctypes.data_as(C.POINTER(C.c_int)),
                                                      C.byref(m), tab.ctypes.data_as(C.POINTER(C.c_int)), C.byref(rows)))
        return nc.value, slot[:nc.value].copy(), m.value, tab[:rows.value].copy()

    # ---- trackMono after initialisation in one step (ov2_btracker_track_mono) --------------------------------------------------
    def setPose(self, item, Twc):
        """the frame pose of item `item` (pcurframe_->Twc_), resident on the device: the estimator or the loop closer moved the frame.
        Between steps only."""
        T = np.ascontiguousarray(Twc, np.float64).reshape(7)
        L.check(self.lib.ov2_btracker_set_pose(self.h_trk, int(item), _ptr(T)))

    def getPose(self, item):
        T = np.zeros(7)
        L.check(self.lib.ov2_btracker_get_pose(self.h_trk, int(item), _ptr(T)))
        return T

    def resetMotion(self, item):
        """MotionModel::reset() of item `item`"""
        L.check(self.lib.ov2_btracker_reset_motion(self.h_trk, int(item)))

    def getMotion(self, item):
        """the motion state of item `item` as motion.apply takes it"""
        from . import motion as _motion
        s = L.MotionState()
        L.check(self.lib.ov2_btracker_get_motion(self.h_trk, int(item), C.byref(s)))
        return _motion._state_dict(s)

    def setKeyframeInfo(self, item, kf_id, kf_time, kf_nb3dkps):
        """id_, img_time_ and nb3dkps_ of the keyframe setKeyframe gave item `item`"""
        L.check(self.lib.ov2_btracker_set_keyframe_info(self.h_trk, int(item), int(kf_id), float(kf_time), int(kf_nb3dkps)))

    def trackMono(self, imgs, kps, wpt, is3d, n, params, epi_params, p3p_req, seed, lmid, nbkfs, epi_seed, time, frame_id,
                  localba_is_on=None, doepipolar=True, scale=None, dop3p=False, n_rows=0, klt_use_prior=True):
        """VisualFrontEnd::trackMono after initialisation in one enqueue and one synchronisation (ov2_btracker_track_mono): the motion
        model on the resident pose (setPose / getPose) and state (resetMotion / getMotion), trackFrameEpiPose (doepipolar False:
        trackFramePose) from the predicted pose, updateMotionModel and checkNewKfReq against the resident keyframe (setKeyframe,
        setKeyframeInfo).  As trackFrameEpiPose without Tcw and Twc, plus time, frame_id and localba_is_on one per item.
        -> (out, status bits, p3p_req, epis (None with doepipolar False), poses, monos): monos[b] = dict(Twc_pred (7,), resynced,
        state (the motion state after the update), kf (as keyframe.kf_decision returns it))."""
        return self._whole(self._marshal_track_mono(imgs, kps, wpt, is3d, n, params, epi_params, p3p_req, seed, lmid, nbkfs, epi_seed, time,
                                                    frame_id, localba_is_on, doepipolar, scale, dop3p, n_rows, klt_use_prior))

    def trackMonoBegin(self, imgs, kps, wpt, is3d, n, params, epi_params, p3p_req, seed, lmid, nbkfs, epi_seed, time, frame_id,
                       localba_is_on=None, doepipolar=True, scale=None, dop3p=False, n_rows=0, klt_use_prior=True):
        """first half of trackMono; trackMonoEnd finishes it (trackFrameEnd gives the tracking half, drops the rest and leaves the
        resident pose and state as they were)"""
        self._begin(self._marshal_track_mono(imgs, kps, wpt, is3d, n, params, epi_params, p3p_req, seed, lmid, nbkfs, epi_seed, time,
                                             frame_id, localba_is_on, doepipolar, scale, dop3p, n_rows, klt_use_prior))

    def trackMonoEnd(self):
        """second half of trackMono -> (out, status bits, p3p_req, epis, poses, monos)"""
        return self._end("track_mono")

    # ---- the current frame resident on the device between the steps (ov2_btracker_set_frame, ..._track_mono_resident) -------------
    def setFrame(self, item, px, lmid, is3d, wpt):
        """installs the current frame of item `item` on the device (ov2_btracker_set_frame): px (n, 2), lmid (n,) distinct and >= 0,
        is3d (n,), wpt (n, 3), n <= n_max.  The first install, and the fallback where createKeyframe did not create.  Between
        steps only."""
        px = np.ascontiguousarray(px, np.float32).reshape(-1, 2)
        lm = np.ascontiguousarray(lmid, np.int32).reshape(-1)
        d3 = np.ascontiguousarray(is3d, np.uint8).reshape(-1)
        w = np.ascontiguousarray(wpt, np.float64).reshape(-1, 3)
        if not (len(px) == len(lm) == len(d3) == len(w)):
            raise ValueError("one px, one lmid, one is3d and one wpt per slot")
        L.check(self.lib.ov2_btracker_set_frame(self.h_trk, int(item), len(lm), _ptr(px), _ptr(lm), _ptr(d3), _ptr(w)))

    def getFrame(self, item, from_device=True):
        """the resident frame of item `item` -> dict(n, px (n, 2), lmid (n,), is3d (n,), wpt (n, 3)): copied down from the device
        block, or with from_device False the host mirror.  wpt of a slot that is not 3-D is whatever the slot last carried."""
        n = C.c_int()
        px, lm = np.zeros((self.n_max, 2), np.float32), np.zeros(self.n_max, np.int32)
        d3, w = np.zeros(self.n_max, np.uint8), np.zeros((self.n_max, 3), np.float64)
        L.check(self.lib.ov2_btracker_get_frame(self.h_trk, int(item), int(bool(from_device)), C.byref(n), _ptr(px), _ptr(lm), _ptr(d3), _ptr(w)))
        k = n.value
        return dict(n=k, px=px[:k].copy(), lmid=lm[:k].copy(), is3d=d3[:k].copy(), wpt=w[:k].copy())

    def updateFrame(self, n_active, ops):
        """what the map did to the resident frames of items [0, n_active) since the last step (ov2_btracker_update_frame_batch), one
        upload, one launch, one download: ops[b] is a list of (lmid, op, xyz) with op L.OV2_RES_SET_POINT (wpt = xyz, is3d = 1),
        L.OV2_RES_UNSET_POINT (is3d = 0) or L.OV2_RES_REMOVE (the slot leaves, the rest close up in slot order); xyz may be None
        where the op does not read it.  An lmid the frame does not hold is counted.
        -> [dict(n_before, n_after, n_set, n_unset, n_removed, n_missing)] per item"""
        na = int(n_active)
        if len(ops) < na:
            raise ValueError("one op list per active item")
        lists, cnt = [], np.zeros(max(1, na), np.int32)
        ptrs = (C.POINTER(L.ResidentOp) * max(1, na))()
        for b in range(na):
            arr = (L.ResidentOp * max(1, len(ops[b])))()
            for j, (lmid, op, xyz) in enumerate(ops[b]):
                arr[j].lmid, arr[j].op = int(lmid), int(op)
                arr[j].xyz = (C.c_double * 3)(*([0.0, 0.0, 0.0] if xyz is None else [float(v) for v in xyz]))
            lists.append(arr)
            cnt[b] = len(ops[b])
            ptrs[b] = C.cast(arr, C.POINTER(L.ResidentOp))
        R = (L.ResidentUpdateResult * max(1, na))()
        L.check(self.lib.ov2_btracker_update_frame_batch(self.h_trk, na, cnt.ctypes.data_as(C.POINTER(C.c_int)), ptrs, R))
        return [{k: int(getattr(R[b], k)) for k, _ in L.ResidentUpdateResult._fields_} for b in range(na)]

    def lastSlotBytes(self):
        """bytes of per-slot input (keypoints, points, flags, ids, scales: anything sized by n or n_max; not images) the last step or
        createKeyframe call wrote for the device: 0 for the resident forms"""
        v = C.c_size_t()
        L.check(self.lib.ov2_btracker_last_slot_bytes(self.h_trk, C.byref(v)))
        return int(v.value)

    def trackMonoResident(self, imgs, params, epi_params, p3p_req, seed, nbkfs, epi_seed, time, frame_id, localba_is_on=None,
                          doepipolar=True, dop3p=False, n_rows=0, klt_use_prior=True):
        """trackMono on the resident frames (ov2_btracker_track_mono_resident): as trackMono without kps, wpt, is3d, n, lmid and scale
        -- the frame of each item is the one setFrame / updateFrame / createKeyframe / the last step left on the device, and the
        step leaves its successor there: the tracked px of the slots that are tracked and were removed by neither the filter nor the
        pose, with their lmid, is3d and wpt, in slot order.
        -> (out, status bits, p3p_req, epis, poses, monos, frames): as trackMono, in the slot space of the frame BEFORE the step;
        frames[b] = dict(n_before, n_after)."""
        return self._whole(self._marshal_track_mono_resident(imgs, params, epi_params, p3p_req, seed, nbkfs, epi_seed, time, frame_id,
                                                             localba_is_on, doepipolar, dop3p, n_rows, klt_use_prior))

    def trackMonoResidentBegin(self, imgs, params, epi_params, p3p_req, seed, nbkfs, epi_seed, time, frame_id, localba_is_on=None,
                               doepipolar=True, dop3p=False, n_rows=0, klt_use_prior=True):
        """first half of trackMonoResident; trackMonoResidentEnd finishes it (trackFrameEnd gives the tracking half, drops the rest and
        leaves the resident pose, state and frames as they were)"""
        self._begin(self._marshal_track_mono_resident(imgs, params, epi_params, p3p_req, seed, nbkfs, epi_seed, time, frame_id,
                                                      localba_is_on, doepipolar, dop3p, n_rows, klt_use_prior))

    def trackMonoResidentEnd(self):
        """second half of trackMonoResident -> (out, status bits, p3p_req, epis, poses, monos, frames)"""
        return self._end("track_mono_resident")

    # ---- createKeyframe for the items a step flagged (ov2_btracker_create_keyframe) ------------------------------------------------
    def createKeyframe(self, n_active, px, lmid, is3d, n, make_kf, nlmid, nkfid, time, params, state, Twc=None, out=None):
        """MapManager::createKeyframe for the items of [0, n_active) with make_kf[b] != 0, in one enqueue and one synchronisation
        (ov2_btracker_create_keyframe): describeBRIEF, the detector's top-up of the empty cells, addKeypointsToFrame, computeKeypoint and
        the new frame installed as the item's resident keyframe (setKeyframe + setKeyframeInfo) without leaving the device.
        px (batch, n_max, 2), lmid / is3d (batch, n_max), n: the current frame after prepareFrame; nlmid, nkfid, time: one per item;
        params: dict(ncellsize, nbwcells, nbhcells, nbmaxkps, detector "singlescale" | "gridfast", det_cell, roi, mask_mode, do_subpix,
        use_brief); state: float64 qualities (single scale) or int32 thresholds (FAST), one per item, updated in place; Twc
        (>= n_active, 7) or None: the resident pose; out: dict of arrays to scatter into (missing ones are zeros).
        px None (with lmid, is3d and n None): the frames are the resident ones (setFrame, trackMonoResident); nothing per slot
        goes up, and the frame with the new points appended (is3d 0, wpt 0) becomes the resident frame of every CREATED item.
        -> (records, out): records[b] = dict(action, n_prev, noccupcells, nb2detect, n_new, n_kf, nb3dkps); out = dict(px, lmid, unpx,
        bv, desc, valid, color) in slot layout, written for the items with action OV2_CKF_CREATED only."""
        return self._whole(self._marshal_create_keyframe(n_active, px, lmid, is3d, n, make_kf, nlmid, nkfid, time, params, state, Twc), out)

    def createKeyframeBegin(self, n_active, px, lmid, is3d, n, make_kf, nlmid, nkfid, time, params, state, Twc=None):
        """first half of createKeyframe: enqueue and return; createKeyframeEnd finishes it (state is updated there: keep it alive)"""
        self._begin(self._marshal_create_keyframe(n_active, px, lmid, is3d, n, make_kf, nlmid, nkfid, time, params, state, Twc))

    def createKeyframeEnd(self, out=None):
        """second half of createKeyframe -> (records, out)"""
        return self._end("create_keyframe", out)

    # ---- the mapper's stereo block on the resident keyframe (ov2_btracker_stereo_keyframe) -----------------------------------------
    def stereoKeyframe(self, n_active, right_pyr, do, params, out=None):
        """MapManager::stereoMatching, then Mapper::triangulateStereo, on the resident keyframe of the items of [0, n_active) with
        do[b] != 0 (normally: the item's last createKeyframe action was OV2_CKF_CREATED), in one enqueue and one synchronisation
        (ov2_btracker_stereo_keyframe): the stereo priors, the line search (rect), the tracking from cur_pyr into right_pyr, the
        epipolar gate, the right camera's computeKeypoint, triangulateStereo; every OV2_TRI_STEREO_OK slot becomes 3-D in the
        resident frame and the keyframe info's kf_nb3dkps is recounted.  right_pyr: a batch Pyramid of the right images on this
        tracker's context (it may still be building); params: mapper.stereo_keyframe_params(...); out: dict of arrays to scatter
        into (missing ones are zeros).  Keypoints of a grid cell stand in slot order (not vgridkps_ insertion order); state 2
        cannot occur (remove such observations with updateFrame first); triangulateTemporal is not run.
        -> (records, out): records[b] = dict(action L.OV2_SKF_*, n, n_prior3d, n_prior_nb, n_stereo_kps, n_stereo, n_stereo_good,
        nb3dkps); out = dict(right_px, stereo_ok, tri_status, wpt, invdepth) in the slot layout of the resident frame, written
        for the items with action OV2_SKF_DONE only."""
        return self._whole(self._marshal_stereo_keyframe(n_active, right_pyr, do, params), out)

    def stereoKeyframeBegin(self, n_active, right_pyr, do, params):
        """first half of stereoKeyframe: enqueue and return; stereoKeyframeEnd finishes it"""
        self._begin(self._marshal_stereo_keyframe(n_active, right_pyr, do, params))

    def stereoKeyframeEnd(self, out=None):
        """second half of stereoKeyframe -> (records, out)"""
        return self._end("stereo_keyframe", out)

    def getKeyframeInfo(self, item, from_device=False):
        """the resident keyframe info of item `item` -> dict(kf_id, kf_time, kf_nb3dkps, has_info): the host mirror, or with
        from_device True copied down from the device block"""
        i, t, n, hi = C.c_int(), C.c_double(), C.c_int(), C.c_int()
        L.check(self.lib.ov2_btracker_get_keyframe_info(self.h_trk, int(item), int(bool(from_device)), C.byref(i), C.byref(t), C.byref(n),
                                                        C.byref(hi)))
        return dict(kf_id=i.value, kf_time=t.value, kf_nb3dkps=n.value, has_info=hi.value)

    # ---- Mapper::triangulateTemporal on the resident keyframe (ov2_btracker_temporal_keyframe) and the anchor table -----------------
    def reserveAnchors(self, n_src_max):
        """allocates the anchor block with n_src_max rows per item (ov2_btracker_reserve_anchors); the first temporalKeyframe does
        it otherwise.  Another n_src_max afterwards is refused."""
        L.check(self.lib.ov2_btracker_reserve_anchors(self.h_trk, int(n_src_max)))
        self._n_src_max = int(n_src_max)

    def setAnchors(self, item, lmid, kfid, unpx, bv, row_kfid, row_Twc):
        """installs the whole anchor table of item `item` (ov2_btracker_set_anchors), as setKeyframe installs a keyframe: per keypoint
        of the latest keyframe lmid (n,) strictly ascending, kfid (n,) its first observing keyframe, unpx (n, 2) and bv (n, 3) its
        keypoint there; per keyframe referred to row_kfid (r,) strictly ascending and row_Twc (r, 7).  After the map culled a
        keyframe, or for a tracker that joins a running map.  Between steps only."""
        lm = np.ascontiguousarray(lmid, np.int32).reshape(-1)
        kf = np.ascontiguousarray(kfid, np.int32).reshape(-1)
        un = np.ascontiguousarray(unpx, np.float32).reshape(-1, 2)
        b = np.ascontiguousarray(bv, np.float64).reshape(-1, 3)
        rk = np.ascontiguousarray(row_kfid, np.int32).reshape(-1)
        rT = np.ascontiguousarray(row_Twc, np.float64).reshape(-1, 7)
        if not (len(lm) == len(kf) == len(un) == len(b)) or len(rk) != len(rT):
            raise ValueError("one kfid, unpx and bv per lmid, one pose per row")
        L.check(self.lib.ov2_btracker_set_anchors(self.h_trk, int(item), len(lm), _ptr(lm), _ptr(kf), _ptr(un), _ptr(b), len(rk), _ptr(rk), _ptr(rT)))

    def getAnchors(self, item, from_device=False):
        """the anchor table of item `item` -> dict(n, lmid (n,), kfid (n,), unpx (n, 2), bv (n, 3), n_rows, row_kfid (r,), row_Twc (r, 7),
        row_Tcw (r, 7)): the host mirror, or with from_device True copied down from the device block"""
        ns = self._n_src_max
        n, nr = C.c_int(), C.c_int()
        lm, kf = np.zeros(self.n_max, np.int32), np.zeros(self.n_max, np.int32)
        un, b = np.zeros((self.n_max, 2), np.float32), np.zeros((self.n_max, 3), np.float64)
        rk, rT, rI = np.zeros(ns, np.int32), np.zeros((ns, 7), np.float64), np.zeros((ns, 7), np.float64)
        L.check(self.lib.ov2_btracker_get_anchors(self.h_trk, int(item), int(bool(from_device)), C.byref(n), _ptr(lm), _ptr(kf), _ptr(un), _ptr(b),
                                                  C.byref(nr), _ptr(rk), _ptr(rT), _ptr(rI)))
        k, r = n.value, nr.value
        return dict(n=k, lmid=lm[:k].copy(), kfid=kf[:k].copy(), unpx=un[:k].copy(), bv=b[:k].copy(), n_rows=r, row_kfid=rk[:r].copy(),
                    row_Twc=rT[:r].copy(), row_Tcw=rI[:r].copy())

    def setAnchorPoses(self, triples):
        """the poses local BA moved (ov2_btracker_set_anchor_poses_batch): triples is a list of (item, kfid, Twc (7,)); one upload and
        one launch for all of them.  -> the number of triples whose kfid anchors nothing in its item (ignored)"""
        it = np.ascontiguousarray([t[0] for t in triples], np.int32).reshape(-1)
        kf = np.ascontiguousarray([t[1] for t in triples], np.int32).reshape(-1)
        T = np.ascontiguousarray([t[2] for t in triples], np.float64).reshape(-1, 7)
        ign = C.c_int()
        L.check(self.lib.ov2_btracker_set_anchor_poses_batch(self.h_trk, len(it), _ptr(it), _ptr(kf), _ptr(T), C.byref(ign)))
        return ign.value

    def temporalKeyframe(self, n_active, do, params, out=None):
        """Mapper::triangulateTemporal on the resident keyframe of the items of [0, n_active) with do[b] != 0 (normally: the item's
        last createKeyframe action was OV2_CKF_CREATED; in stereo behind stereoKeyframe), in one enqueue and one synchronisation
        (ov2_btracker_temporal_keyframe): the item's anchor table moves on to this keyframe, every 2-D slot the keyframe holds whose
        anchor is an earlier keyframe is triangulated against it, every OV2_TRI_TEMPORAL_OK slot becomes 3-D in the resident
        frame, every OV2_TRI_REMOVE_OBS slot leaves the resident keyframe, kf_nb3dkps is recounted.  params:
        mapper.temporal_keyframe_params(...); out: dict of arrays to scatter into (missing ones are zeros).  Points first seen at a
        keyframe for which this call was not run anchor at the next one for which it is.
        -> (records, out): records[b] = dict(action L.OV2_TKF_*, n, n_candidates, n_temporal_good, n_remove_obs, n_no_motion, nb3dkps,
        n_rows); out = dict(tri_status, wpt, invdepth, src_kfid) in the slot layout of the resident frame, written for the items with
        action OV2_TKF_DONE only."""
        res = self._whole(self._marshal_temporal_keyframe(n_active, do, params), out)
        self._n_src_max = int(params.n_src_max)
        return res

    def temporalKeyframeBegin(self, n_active, do, params):
        """first half of temporalKeyframe: enqueue and return; temporalKeyframeEnd finishes it"""
        self._begin(self._marshal_temporal_keyframe(n_active, do, params))
        self._n_src_max = int(params.n_src_max)

    def temporalKeyframeEnd(self, out=None):
        """second half of temporalKeyframe -> (records, out)"""
        return self._end("temporal_keyframe", out)

    # ---- trackMono's un-initialised branch on the resident frame and keyframe (ov2_btracker_mono_init) ----------------------------------
    def monoInit(self, n_active, do, seed, params, out=None):
        """checkReadyForInit for the items with do[b] != 0, right after their trackMonoResident step, on the resident frame, pose and
        keyframe (ov2_btracker_mono_init): one enqueue, no per-slot byte goes up.  Where the action is MINIT_READY the removed slots
        leave the resident frame and the resident pose becomes Twc_init (the pose of the UNREFINED model: pose_refined = 0); the
        motion state of every item that ran is reset.  seed: one per item, of the sample table; params:
        keyframe.mono_init_params(...) or the dict of them; out: dict with `removed` to scatter into (missing: zeros).
        -> (records, out): records[b] is the dict of keyframe.mono_init without its arrays (action L.OV2_MINIT_*, NOT_REQUESTED and
        NO_KEYFRAME among them); out["removed"] (batch, n_max) uint8"""
        return self._whole(self._marshal_mono_init(n_active, do, seed, params), out)

    def monoInitBegin(self, n_active, do, seed, params):
        """first half of monoInit: enqueue and return; monoInitEnd finishes it"""
        self._begin(self._marshal_mono_init(n_active, do, seed, params))

    def monoInitEnd(self, out=None):
        """second half of monoInit -> (records, out)"""
        return self._end("mono_init", out)

    def lastPriors(self, item, n):
        """(prior (n, 2) float32, has_prior (n,) uint8) of item `item` as the last step used them"""
        pri = np.empty((n, 2), np.float32)
        hp = np.empty(n, np.uint8)
        L.check(self.lib.ov2_btracker_last_priors(self.h_trk, int(item), int(n), _ptr(pri), _ptr(hp)))
        return pri, hp

    def lastKeypoints(self, item, n, want_bv=True):
        unpx = np.empty((n, 2), np.float32)
        bv = np.empty((n, 3), np.float64) if want_bv else None
        L.check(self.lib.ov2_btracker_last_keypoints(self.h_trk, int(item), int(n), _ptr(unpx), _ptr(bv) if want_bv else None))
        return unpx, bv

    def describeBRIEF(self, n_active, pts, n):
        """describeBRIEF on the raw frames of the current step, items [0, n_active).  pts: (>= n_active, cap, 2) float32; n: counts
        (len n_active).  -> (desc (n_active, cap, 32) uint8, valid (n_active, cap) bool; slots past n[b] are zero).  Call it before
        the staging set of those frames is uploaded or prepared again."""
        na = int(n_active)
        p = np.asarray(pts, np.float32)
        if p.ndim != 3 or p.shape[0] < na or p.shape[2] != 2:
            raise ValueError("pts must be (>= n_active, cap, 2)")
        cap = p.shape[1]
        p = np.ascontiguousarray(p[:na])
        nn = np.ascontiguousarray(n, np.int32)
        if len(nn) != na:
            raise ValueError("one point count per active item")
        desc = np.zeros((na, cap, L.OV2_BRIEF_BYTES), np.uint8); valid = np.zeros((na, cap), np.uint8)
        L.check(self.lib.ov2_btracker_describe_brief(self.h_trk, na, _ptr(p), _ptr(nn), cap, _ptr(desc), _ptr(valid)))
        return desc, valid.astype(bool)

    def detectSingleScale(self, n_active, ncellsize, cur, ncur, roi, quality, subpix=True):
        """MapManager::extractKeypoints of items [0, n_active) on their current frames.  cur: (batch, n_max, 2); ncur: counts;
        quality: float64 array, one dmaxquality_ per item, updated in place.  -> list of (k, 2) arrays"""
        cap = max(1, 2 * (self.w // ncellsize) * (self.h // ncellsize))
        cur = np.ascontiguousarray(cur, np.float32).reshape(self.batch, self.n_max, 2)
        nc = np.ascontiguousarray(ncur, np.int32)
        q = np.ascontiguousarray(quality, np.float64)
        assert q is quality or np.shares_memory(q, quality), "quality must be a contiguous float64 array (updated in place)"
        out = np.zeros((n_active, cap, 2), np.float32); on = np.zeros(n_active, np.int32)
        r = (C.c_int * 4)(*[int(v) for v in roi])
        L.check(self.lib.ov2_btracker_detect_singlescale(self.h_trk, int(n_active), int(ncellsize), _ptr(cur), _ptr(nc), r, _ptr(q),
                                                         1 if subpix else 0, _ptr(out), cap, _ptr(on)))
        return [out[b, :on[b]].copy() for b in range(n_active)]

    def detectGFTT(self, n_active, params, cur, ncur, nbmax, roi=None, subpix=True):
        """detectGFTT of items [0, n_active) on their current frames.  params: L.GfttParams (FeatureExtractor.gftt_params());
        cur: (batch, n_max, 2); ncur / nbmax: one per active item; roi None or an (h, w) uint8 mask shared by the items.
        -> list of (k, 2) arrays"""
        cur = np.ascontiguousarray(cur, np.float32).reshape(self.batch, self.n_max, 2)
        nc = np.zeros(self.batch, np.int32); nc[:n_active] = np.asarray(ncur, np.int32)[:n_active]
        nb = np.ascontiguousarray(nbmax, np.int32)
        cap = max([1] + [int(v) if v != -1 else params.nmaxpts for v in nb[:n_active]])
        r, rp, rs = _roi_arg(roi, self.w, self.h)
        out = np.zeros((n_active, cap, 2), np.float32); on = np.zeros(n_active, np.int32)
        L.check(self.lib.ov2_btracker_detect_gftt(self.h_trk, int(n_active), rp, rs, C.byref(params), _ptr(cur), _ptr(nc), _ptr(nb),
                                                  1 if subpix else 0, _ptr(out), cap, _ptr(on)))
        return [out[b, :on[b]].copy() for b in range(n_active)]

    def detectGridFAST(self, n_active, ncellsize, cur, ncur, fast_th, mask_mode=L.OV2_MASK_AS_EXECUTED, subpix=True):
        cap = max(1, (self.w // ncellsize) * (self.h // ncellsize))
        cur = np.ascontiguousarray(cur, np.float32).reshape(self.batch, self.n_max, 2)
        nc = np.ascontiguousarray(ncur, np.int32)
        t = np.ascontiguousarray(fast_th, np.int32)
        assert t is fast_th or np.shares_memory(t, fast_th), "fast_th must be a contiguous int32 array (updated in place)"
        out = np.zeros((n_active, cap, 2), np.float32); on = np.zeros(n_active, np.int32)
        L.check(self.lib.ov2_btracker_detect_grid_fast(self.h_trk, int(n_active), int(ncellsize), _ptr(cur), _ptr(nc), _ptr(t), int(mask_mode),
                                                       1 if subpix else 0, _ptr(out), cap, _ptr(on)))
        return [out[b, :on[b]].copy() for b in range(n_active)]

    @property
    def cur_pyr(self):
        """the current frame's pyramids, all items (e.g. `left` of stereo.stereo_match_batch_arrays)"""
        v = _PyrView(self.ctx, C.c_void_p(self.lib.ov2_btracker_cur_pyr(self.h_trk)), self.w, self.h, self.win)
        v.batch = self.batch
        return v

    def cur_item(self, item):
        return _PyrView(self.ctx, C.c_void_p(self.lib.ov2_btracker_cur_item(self.h_trk, int(item))), self.w, self.h, self.win)

    def prev_item(self, item):
        return _PyrView(self.ctx, C.c_void_p(self.lib.ov2_btracker_prev_item(self.h_trk, int(item))), self.w, self.h, self.win)

    # ---- tracking from the keyframe: VisualFrontEnd::kltTrackingFromKF (ov2_btracker_set_track_from_keyframe) ----------------------
    def setTrackFromKeyframe(self, on=True):
        """btrack_keyframetoframe: while on, trackFrameEpiPose, trackMono and trackMonoResident track every frame from the item's last
        keyframe -- its pyramid in the tracker's keyframe store, its px from the keyframe-px table, joined by lmid -- instead of the
        previous frame, and createKeyframe adopts the pyramid and installs the table of every item it creates.  status 4 marks a
        slot the keyframe no longer holds.  The first call allocates the store.  Between steps only."""
        L.check(self.lib.ov2_btracker_set_track_from_keyframe(self.h_trk, 1 if on else 0))

    def adoptKeyframePyramid(self, n_active, do):
        """the current pyramid of every item b < n_active with do[b] becomes its keyframe pyramid (ov2_btracker_adopt_keyframe_pyramid):
        for keyframes built on the host.  Between steps only."""
        d = np.zeros(max(1, int(n_active)), np.uint8)
        d[:int(n_active)] = np.asarray(do, np.uint8).reshape(-1)[:int(n_active)] != 0
        L.check(self.lib.ov2_btracker_adopt_keyframe_pyramid(self.h_trk, int(n_active), _ptr(d)))

    def setKeyframePx(self, item, lmid, px):
        """the keyframe-px table of item `item` (ov2_btracker_set_keyframe_px): lmid (n,) strictly ascending, px (n, 2) finite, the
        keyframe's distorted pixel of every id."""
        lm = np.ascontiguousarray(lmid, np.int32).reshape(-1)
        px = np.ascontiguousarray(px, np.float32).reshape(-1, 2)
        if len(lm) != len(px):
            raise ValueError("one px per lmid")
        L.check(self.lib.ov2_btracker_set_keyframe_px(self.h_trk, int(item), len(lm), _ptr(lm), _ptr(px)))

    def getKeyframePx(self, item, from_device=True):
        """the keyframe-px table of item `item` -> dict(n, lmid (n,), px (n, 2)), from the device or the host mirror"""
        n = C.c_int()
        lm, px = np.zeros(self.n_max, np.int32), np.zeros((self.n_max, 2), np.float32)
        L.check(self.lib.ov2_btracker_get_keyframe_px(self.h_trk, int(item), int(bool(from_device)), C.byref(n), _ptr(lm), _ptr(px)))
        k = n.value
        return dict(n=k, lmid=lm[:k].copy(), px=px[:k].copy())

    def kf_item(self, item):
        """item `item` of the keyframe store as a batch-1 pyramid view (None before the first setTrackFromKeyframe)"""
        h = self.lib.ov2_btracker_kf_item(self.h_trk, int(item))
        return _PyrView(self.ctx, C.c_void_p(h), self.w, self.h, self.win) if h else None

    def close(self):
        if getattr(self, "h_trk", None):
            self.image_buffers = None
            self.lib.ov2_btracker_destroy(self.h_trk)
            self.h_trk = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
