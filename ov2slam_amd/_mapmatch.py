"""Plumbing shared by the wrappers of the two local-map matchers (csrc/mapmatch.hip): Mapper::matchToMap in mapper.py and
LoopCloser::matchToMap in loop_closer.py.  The two call families have their own C types, whose params and result structs hold the
same fields and whose item structs differ in a few tables; a Family binds one set of types to the code below."""
import ctypes as C

import numpy as np

from . import _lib as L

CAM_MODELS = {"pinhole": L.OV2_CAM_PINHOLE, "fisheye": L.OV2_CAM_FISHEYE}
_PARAM_KEYS = ("K", "D", "model", "img_w", "img_h", "ncellsize", "fmax_proj_pxdist", "fmax_desc_dist", "desc_bytes")
_PER_KP = (("kp_px", 2), ("kp_matched", 1))                  # elements per keypoint / per observation, where the family has the table
_PER_OBS = (("obs_kfid", 1), ("obs_kf", 1), ("obs_px", 2))


def _p(a, ct):
    return a.ctypes.data_as(C.POINTER(ct)) if a is not None and a.size else None


class Family:
    def __init__(self, name, single, batch, params_t, item_t, result_t, fields, scalars=(), defaults=()):
        """name: the prefix of the ValueError texts; single / batch: the library's two functions; fields: (name, numpy dtype, ctypes
        type) of the item's arrays; scalars: its plain int fields; defaults: of the optional keys of a params dict"""
        self.name, self.single, self.batch = name, single, batch
        self.params_t, self.item_t, self.result_t, self.fields, self.scalars = params_t, item_t, result_t, fields, scalars
        self.defaults = dict(D=None, model="pinhole", desc_bytes=32, **dict(defaults))

    def params(self, K, D, model, img_w, img_h, ncellsize, fmax_proj_pxdist, fmax_desc_dist, desc_bytes):
        """the params struct; it keeps its distortion array alive"""
        p = self.params_t()
        p.model = CAM_MODELS[model] if isinstance(model, str) else int(model)
        p.K[:] = [float(v) for v in np.asarray(K, np.float64).reshape(4)]
        d = np.zeros(0) if D is None else np.ascontiguousarray(D, np.float64).reshape(-1)
        p._D = d
        p.D, p.nD = _p(d, C.c_double), int(d.size)
        p.img_w, p.img_h, p.ncellsize = float(img_w), float(img_h), int(ncellsize)
        p.fmax_proj_pxdist, p.fmax_desc_dist, p.desc_bytes = float(fmax_proj_pxdist), float(fmax_desc_dist), int(desc_bytes)
        return p

    def as_params(self, params):
        if isinstance(params, self.params_t):
            return params
        return self.params(*(params[k] if k in params or k not in self.defaults else self.defaults[k] for k in _PARAM_KEYS))

    def item(self, item):
        """(the item struct, the arrays it points into, n_lm, n_kp); the counts are taken from the array lengths"""
        t = np.ascontiguousarray(item["Tcw"], dtype=np.float64)
        if t.size != 7:
            raise ValueError("%s: Tcw must hold 7 doubles (translation, then the quaternion x y z w)" % self.name)
        keep = dict(Tcw=t)
        s = self.item_t()
        s.Tcw = _p(t, C.c_double)
        for f in self.scalars:
            setattr(s, f, int(item[f]))
        for name, dt, ct in self.fields:
            a = item.get(name)
            a = None if a is None else np.ascontiguousarray(a, dtype=dt)
            keep[name] = a
            setattr(s, name, _p(a, ct))
        size = lambda n: 0 if keep[n] is None else keep[n].size
        s.n_kp, s.n_lm = size("kp_mp"), size("lm_mp")
        s.n_mp = max(size("obs_start") - 1, 0)
        if "kf_Tcw" in keep:
            s.n_kf = size("kf_Tcw") // 7
        per_kp = [(n, w) for n, w in _PER_KP if n in keep]
        per_obs = [(n, w) for n, w in _PER_OBS if n in keep]
        if any(size(n) != w * s.n_kp for n, w in per_kp) or size("lm_wpt") != 3 * s.n_lm or size("desc_start") != size("obs_start"):
            raise ValueError("%s: array lengths disagree (%s / kp_mp, lm_wpt / lm_mp, obs_start / desc_start)"
                             % (self.name, " / ".join(n for n, _ in per_kp)))
        if s.n_mp and (any(size(n) != w * keep["obs_start"][-1] for n, w in per_obs) or size("desc") != 32 * keep["desc_start"][-1]):
            raise ValueError("%s: the observation / descriptor arrays are not as long as their offsets say" % self.name)
        if size("cell_start") and size("cell_kp") != keep["cell_start"][-1]:
            raise ValueError("%s: cell_kp is not as long as cell_start says" % self.name)
        return s, keep, s.n_lm, s.n_kp

    def result(self, n_lm, n_kp):
        """(the result struct, the dict of arrays it points into)"""
        out = dict(lm_status=np.zeros(n_lm, np.uint8), lm_kp=np.full(n_lm, -1, np.int32), lm_dist=np.zeros(n_lm, np.float32),
                   lm_projpx=np.zeros((n_lm, 2), np.float32), kp_lm=np.full(n_kp, -1, np.int32), kp_dist=np.zeros(n_kp, np.float32))
        r = self.result_t()
        r.lm_status = _p(out["lm_status"], C.c_uint8)
        r.lm_kp, r.kp_lm = _p(out["lm_kp"], C.c_int), _p(out["kp_lm"], C.c_int)
        r.lm_dist, r.lm_projpx, r.kp_dist = _p(out["lm_dist"], C.c_float), _p(out["lm_projpx"], C.c_float), _p(out["kp_dist"], C.c_float)
        return r, out

    def call(self, ctx, params, item):
        s, keep, n_lm, n_kp = self.item(item)
        r, out = self.result(n_lm, n_kp)
        L.check(getattr(ctx.lib, self.single)(ctx.h, C.byref(self.as_params(params)), C.byref(s), C.byref(r)))
        out["n_matches"] = r.n_matches
        return out

    def call_batch(self, ctx, params, items):
        items = list(items)
        S = (self.item_t * max(1, len(items)))()
        R = (self.result_t * max(1, len(items)))()
        keep, outs = [], []
        for b, item in enumerate(items):
            s, k, n_lm, n_kp = self.item(item)
            r, out = self.result(n_lm, n_kp)
            S[b], R[b] = s, r
            keep.append(k); outs.append(out)
        L.check(getattr(ctx.lib, self.batch)(ctx.h, C.byref(self.as_params(params)), len(items), S, R))
        for b, out in enumerate(outs):
            out["n_matches"] = R[b].n_matches
        return outs
