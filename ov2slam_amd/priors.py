"""Host-side mirror of the places where the reference derives the priors of its KLT calls, on top of the C ABI (ov2_klt_priors /
ov2_stereo_priors and their batch forms, csrc/priors.hip):

    klt_priors      VisualFrontEnd::kltTracking (src/visual_front_end.cpp:156-184): the map point of every 3-D keypoint projected with
                    the predicted pose, kept when it lands in the image
    stereo_priors   MapManager::stereoMatching (src/map_manager.cpp:396-489): the map point projected into the right image and, without
                    rectification, the inverse-distance-weighted depth of the 3-D neighbours pushed through the right camera

Params are dicts: model ("pinhole" / "fisheye"), K (fx fy cx cy), D (or None), img_w, img_h, and klt_use_prior (frame form) or
Tcic0 (7), ncellsize, rect (stereo form, the RIGHT camera).  An item is a dict named like the fields of ov2_klt_priors_item /
ov2_stereo_priors_item, the count following from the array lengths: Tcw (7,), px (n,2), is3d (n,), wpt (n,3); for the stereo form
also unpx (n,2), bv (n,3), state (n,) and the cell tables cell_start / cell_kp of ov2_match_keyframe.  Poses are [tx ty tz qx qy qz
qw]; Tcw is the predicted pose, already inverted.  The stereo result's prior / has_prior are what stereo.stereo_match takes as its
3-D priors."""
import ctypes as C

import numpy as np

from . import _lib as L
from ._mapmatch import CAM_MODELS, _p

_KLT_FIELDS = (("px", np.float32, C.c_float, 2), ("is3d", np.uint8, C.c_uint8, 1), ("wpt", np.float64, C.c_double, 3))
_STEREO_FIELDS = (("px", np.float32, C.c_float, 2), ("unpx", np.float32, C.c_float, 2), ("bv", np.float64, C.c_double, 3),
                  ("wpt", np.float64, C.c_double, 3), ("state", np.uint8, C.c_uint8, 1))


def _camera(p, params):
    model = params.get("model", "pinhole")
    p.model = CAM_MODELS[model] if isinstance(model, str) else int(model)
    p.K[:] = [float(v) for v in np.asarray(params["K"], np.float64).reshape(4)]
    d = np.zeros(0) if params.get("D") is None else np.ascontiguousarray(params["D"], np.float64).reshape(-1)
    p._D = d                                                            # the struct keeps its distortion array alive
    p.D, p.nD = _p(d, C.c_double), int(d.size)
    p.img_w, p.img_h = float(params["img_w"]), float(params["img_h"])
    return p


def _as_klt_params(params):
    if isinstance(params, L.KltPriorsParams):
        return params
    p = _camera(L.KltPriorsParams(), params)
    p.klt_use_prior = int(bool(params.get("klt_use_prior", True)))
    return p


def _as_stereo_params(params):
    if isinstance(params, L.StereoPriorsParams):
        return params
    p = _camera(L.StereoPriorsParams(), params)
    p.Tcic0[:] = [float(v) for v in np.asarray(params["Tcic0"], np.float64).reshape(7)]
    p.ncellsize, p.rect = int(params["ncellsize"]), int(bool(params.get("rect", False)))
    return p


def _item(item, struct_t, fields, name):
    """(the item struct, the arrays it points into)"""
    t = np.ascontiguousarray(item["Tcw"], dtype=np.float64)
    if t.size != 7:
        raise ValueError("%s: Tcw must hold 7 doubles (translation, then the quaternion x y z w)" % name)
    keep = dict(Tcw=t)
    s = struct_t()
    s.Tcw = _p(t, C.c_double)
    s.n = int(np.asarray(item["px"]).size // 2)
    for f, dt, ct, width in fields:
        a = np.ascontiguousarray(item[f], dtype=dt)
        if a.size != width * s.n:
            raise ValueError("%s: %s has %d elements, not %d per keypoint" % (name, f, a.size, width))
        keep[f] = a
        setattr(s, f, _p(a, ct))
    return s, keep


def _klt_item(item):
    return _item(item, L.KltPriorsItem, _KLT_FIELDS, "klt_priors")


def _stereo_item(item):
    s, keep = _item(item, L.StereoPriorsItem, _STEREO_FIELDS, "stereo_priors")
    for f in ("cell_start", "cell_kp"):
        a = item.get(f)
        a = None if a is None else np.ascontiguousarray(a, dtype=np.int32)
        keep[f] = a
        setattr(s, f, a.ctypes.data_as(C.POINTER(C.c_int)) if a is not None and a.size else None)
    cs, ck = keep["cell_start"], keep["cell_kp"]
    if cs is not None and cs.size and (0 if ck is None else ck.size) != cs[-1]:
        raise ValueError("stereo_priors: cell_kp is not as long as cell_start says")
    return s, keep


def _klt_result(n):
    out = dict(prior=np.zeros((n, 2), np.float32), has_prior=np.zeros(n, np.uint8))
    r = L.KltPriorsResult()
    r.prior, r.has_prior = _p(out["prior"], C.c_float), _p(out["has_prior"], C.c_uint8)
    return r, out


def _stereo_result(n):
    out = dict(prior=np.zeros((n, 2), np.float32), has_prior=np.zeros(n, np.uint8), skip=np.zeros(n, np.uint8))
    r = L.StereoPriorsResult()
    r.prior, r.has_prior, r.skip = _p(out["prior"], C.c_float), _p(out["has_prior"], C.c_uint8), _p(out["skip"], C.c_uint8)
    return r, out


def _finish_klt(out, r):
    out["n_prior"] = r.n_prior
    return out


def _finish_stereo(out, r):
    out["n_prior3d"], out["n_prior_nb"], out["n_skip"] = r.n_prior3d, r.n_prior_nb, r.n_skip
    return out


def _batch(ctx, fn, params, items, item_t, result_t, make_item, make_result, finish):
    items = list(items)
    S = (item_t * max(1, len(items)))()
    R = (result_t * max(1, len(items)))()
    keep, outs = [], []
    for b, it in enumerate(items):
        S[b], k = make_item(it)
        R[b], out = make_result(S[b].n)
        keep.append(k); outs.append(out)
    L.check(fn(ctx.h, C.byref(params), len(items), S, R))
    return [finish(out, R[b]) for b, out in enumerate(outs)]


def klt_priors(ctx, params, item):
    """ov2_klt_priors: prior (n,2) float32 (px where there is none), has_prior (n,) uint8, n_prior"""
    s, keep = _klt_item(item)
    r, out = _klt_result(s.n)
    L.check(ctx.lib.ov2_klt_priors(ctx.h, C.byref(_as_klt_params(params)), C.byref(s), C.byref(r)))
    return _finish_klt(out, r)


def klt_priors_batch(ctx, params, items):
    """ov2_klt_priors_batch: the frames of a lock-step batch in one launch (shared params); one dict per item"""
    return _batch(ctx, ctx.lib.ov2_klt_priors_batch, _as_klt_params(params), items, L.KltPriorsItem, L.KltPriorsResult, _klt_item,
                  _klt_result, _finish_klt)


def stereo_priors(ctx, params, item):
    """ov2_stereo_priors: prior (n,2) float32, has_prior (n,) uint8 (0, 1 = map point, 2 = neighbours), skip (n,) uint8 and the
    counts n_prior3d, n_prior_nb, n_skip"""
    s, keep = _stereo_item(item)
    r, out = _stereo_result(s.n)
    L.check(ctx.lib.ov2_stereo_priors(ctx.h, C.byref(_as_stereo_params(params)), C.byref(s), C.byref(r)))
    return _finish_stereo(out, r)


def stereo_priors_batch(ctx, params, items):
    """ov2_stereo_priors_batch: the keyframes of a lock-step batch in one launch (shared params); one dict per item"""
    return _batch(ctx, ctx.lib.ov2_stereo_priors_batch, _as_stereo_params(params), items, L.StereoPriorsItem, L.StereoPriorsResult,
                  _stereo_item, _stereo_result, _finish_stereo)
