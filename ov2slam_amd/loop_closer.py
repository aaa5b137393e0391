"""Host-side mirror of the loop closer's descriptor matching (the reference's LoopCloser::knnMatching, src/loop_closer.cpp:378-459)
on top of the C ABI (ov2_knn_match[_batch], csrc/knn.hip): a brute-force Hamming 2-nearest-neighbour search of every query
descriptor among the train descriptors, the distance gate and the ratio test.

An item is a pair (query, train) of uint8 arrays of shape (n, 32); either may be empty.  A result is a dict: idx (n_query, 2) int32
(train rows of the nearest and the second nearest, -1: none), dist (n_query, 2) int32 (their Hamming distances, -1 where idx is -1),
good (n_query,) uint8, pairs (n_pairs, 2) int32 (query row, train row) of the good rows in query order.  The two frame walks that
collect the rows and their ids (:391-420) stay with the caller, who maps the pairs through vkpids / vlmids.

And of the keyframe preparation in front of it (LoopCloser::run, src/loop_closer.cpp:86-144) on top of ov2_lckf_prepare* (csrc/lckf.hip):
the exclusion mask around the keypoints that are already described, FAST(20) on the whole raw image, retainBest(300) and BRIEF of what
is left.  lckf_prepare returns a dict: n_all, cut, n_kept, n_desc (ints, the true counts), kept_xy (n, 2) int16, kept_resp (n,) uint8,
kept_valid (n,) uint8, kept_desc (n, 32) uint8 in raster order (y, then x) and, with want_all, all_xy / all_resp: the corners before
retainBest.  The frame walk that collects the exclusion points and the vconcat with the existing descriptors stay with the caller.

And of the local-map tracking behind P3P (LoopCloser::trackLoopLocalMap / matchToMap, src/loop_closer.cpp:502-763) on top of
ov2_loop_match_to_map[_batch] (csrc/mapmatch.hip): loopmap_params(), loop_match_to_map(), loop_match_to_map_batch().  An item is a dict
of numpy arrays named like the fields of ov2_loopmap_item (the counts are taken from the array lengths); a result is a dict with
lm_status (n_lm,) uint8 (OV2_LOOPMAP_* bits), lm_kp, lm_dist, lm_projpx (n_lm, 2), kp_lm (n_kp,), kp_dist, n_matches.  The
covisible-keyframe walk that builds the local set and the flattening of the map stay with the caller."""
import ctypes as C

import numpy as np

from . import _lib as L
from . import _mapmatch


def knn_params(desc_bytes=32, max_dist=None, ratio=0.85):
    """ov2_knn_params; max_dist defaults to the reference's int(query.cols * 0.5 * 8.)"""
    p = L.KnnParams()
    p.desc_bytes = int(desc_bytes)
    p.max_dist = int(desc_bytes * 0.5 * 8.) if max_dist is None else int(max_dist)
    p.ratio = float(ratio)
    return p


def _as_params(params):
    if isinstance(params, L.KnnParams):
        return params
    return knn_params(params.get("desc_bytes", 32), params.get("max_dist"), params.get("ratio", 0.85))


def _rows(a, what):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.size == 0:
        return a.reshape(0, 32)
    if a.ndim != 2 or a.shape[1] != 32:
        raise ValueError("knn_match: %s must be an (n, 32) uint8 array" % what)
    return a


def _p(a, ct):
    return a.ctypes.data_as(C.POINTER(ct)) if a.size else None


def _item(query, train):
    """(ov2_knn_item, the arrays it points into)"""
    q, t = _rows(query, "query"), _rows(train, "train")
    s = L.KnnItem()
    s.n_query, s.n_train = len(q), len(t)
    s.query, s.train = _p(q, C.c_uint8), _p(t, C.c_uint8)
    return s, (q, t)


def _result(n_query):
    out = dict(idx=np.full((n_query, 2), -1, np.int32), dist=np.full((n_query, 2), -1, np.int32), good=np.zeros(n_query, np.uint8),
               pair_query=np.zeros(n_query, np.int32), pair_train=np.zeros(n_query, np.int32))
    r = L.KnnResult()
    r.idx, r.dist, r.good = _p(out["idx"], C.c_int), _p(out["dist"], C.c_int), _p(out["good"], C.c_uint8)
    r.pair_query, r.pair_train = _p(out["pair_query"], C.c_int), _p(out["pair_train"], C.c_int)
    return r, out


def _finish(r, out):
    n = r.n_pairs
    out["pairs"] = np.stack([out.pop("pair_query")[:n], out.pop("pair_train")[:n]], axis=1)
    return out


def knn_match(ctx, params, query, train):
    """ov2_knn_match: LoopCloser::knnMatching's matcher, gate and ratio test for one query / train pair"""
    s, keep = _item(query, train)
    r, out = _result(s.n_query)
    L.check(ctx.lib.ov2_knn_match(ctx.h, C.byref(_as_params(params)), C.byref(s), C.byref(r)))
    return _finish(r, out)


def knn_match_batch(ctx, params, items):
    """ov2_knn_match_batch: (query, train) pairs in one call (shared params).  Returns one dict per item, as knn_match."""
    items = list(items)
    S = (L.KnnItem * max(1, len(items)))()
    R = (L.KnnResult * max(1, len(items)))()
    keep, outs = [], []
    for b, (query, train) in enumerate(items):
        s, k = _item(query, train)
        r, out = _result(s.n_query)
        S[b], R[b] = s, r
        keep.append(k); outs.append(out)
    L.check(ctx.lib.ov2_knn_match_batch(ctx.h, C.byref(_as_params(params)), len(items), S, R))
    return [_finish(R[b], out) for b, out in enumerate(outs)]


# ---- keyframe preparation ------------------------------------------------------------------------------------------------------
LCKF_KEPT_CAP = 4096          # first guess of the wrappers; a call that reports more is repeated with the reported count
LCKF_ALL_CAP = 65536


def lckf_params(threshold=20, retain=300, excl_radius=2):
    """ov2_lckf_params; the defaults are the reference's"""
    p = L.LckfParams()
    p.threshold, p.retain, p.excl_radius = int(threshold), int(retain), int(excl_radius)
    return p


def _as_lckf_params(params):
    if isinstance(params, L.LckfParams):
        return params
    return lckf_params(**dict(params or {}))


def _excl(excl_xy):
    e = np.ascontiguousarray(excl_xy if excl_xy is not None else np.zeros((0, 2)), dtype=np.float32)
    if e.size == 0:
        return e.reshape(0, 2)
    if e.ndim != 2 or e.shape[1] != 2:
        raise ValueError("lckf_prepare: excl_xy must be an (n, 2) float array")
    return e


def _image(img):
    im = np.asarray(img)
    if im.dtype != np.uint8 or im.ndim != 2 or im.shape[0] < 1 or im.shape[1] < 1:
        raise ValueError("lckf_prepare: img must be a 2-D uint8 array")
    return im if im.strides[1] == 1 and im.strides[0] >= im.shape[1] else np.ascontiguousarray(im)


def lckf_buffers(kept_cap, all_cap, fill=0):
    """(ov2_lckf_result, dict of the arrays it points into), every byte of the arrays set to `fill`"""
    kept_cap, all_cap = int(kept_cap), int(all_cap)
    if kept_cap < 0 or all_cap < 0:
        raise ValueError("lckf_prepare: negative capacity")
    out = dict(kept_xy=np.full((kept_cap, 2), fill, np.int16), kept_resp=np.full(kept_cap, fill, np.uint8),
               kept_valid=np.full(kept_cap, fill, np.uint8), kept_desc=np.full((kept_cap, L.OV2_BRIEF_BYTES), fill, np.uint8),
               all_xy=np.full((all_cap, 2), fill, np.int16), all_resp=np.full(all_cap, fill, np.uint8))
    for a in out.values():
        a.view(np.uint8)[...] = fill
    r = L.LckfResult()
    r.kept_xy, r.kept_resp = _p(out["kept_xy"], C.c_int16), _p(out["kept_resp"], C.c_uint8)
    r.kept_valid, r.kept_desc, r.kept_cap = _p(out["kept_valid"], C.c_uint8), _p(out["kept_desc"], C.c_uint8), kept_cap
    r.all_xy, r.all_resp, r.all_cap = _p(out["all_xy"], C.c_int16), _p(out["all_resp"], C.c_uint8), all_cap
    return r, out


def _lckf_finish(r, out, want_all):
    nk, na = min(r.n_kept, r.kept_cap), min(r.n_all, r.all_cap)
    res = dict(n_all=r.n_all, cut=r.cut, n_kept=r.n_kept, n_desc=r.n_desc, kept_xy=out["kept_xy"][:nk], kept_resp=out["kept_resp"][:nk],
               kept_valid=out["kept_valid"][:nk], kept_desc=out["kept_desc"][:nk])
    if want_all:
        res.update(all_xy=out["all_xy"][:na], all_resp=out["all_resp"][:na])
    return res


def _lckf_retry(call, want_all, kept_cap, all_cap, raw=False):
    """the call with the given capacities (None: a guess, and once more with the reported counts when the guess was too small)"""
    kc = LCKF_KEPT_CAP if kept_cap is None else int(kept_cap)
    ac = (LCKF_ALL_CAP if all_cap is None else int(all_cap)) if want_all else 0
    for _ in range(2):
        rs = call(kc, ac)
        short_k = kept_cap is None and max(r.n_kept for r, _ in rs) > kc
        short_a = want_all and all_cap is None and max(r.n_all for r, _ in rs) > ac
        if not (short_k or short_a):
            break
        kc = max(r.n_kept for r, _ in rs) if short_k else kc
        ac = max(r.n_all for r, _ in rs) if short_a else ac
    res = [_lckf_finish(r, out, want_all) for r, out in rs]
    if raw:                                          # the whole slot arrays, for a caller that checks what lies past the lists
        for f, (_, out) in zip(res, rs):
            f["raw"] = out
    return res


def lckf_prepare(ctx, params, img, excl_xy, want_all=False, kept_cap=None, all_cap=None, fill=0, raw=False):
    """ov2_lckf_prepare on a host image.  kept_cap / all_cap: list capacities (lists are cut there, the counts stay true); None
    sizes them so that nothing is cut.  raw: the dict also carries "raw", the whole slot arrays (pre-set to `fill`)."""
    im, e, p = _image(img), _excl(excl_xy), _as_lckf_params(params)

    def call(kc, ac):
        r, out = lckf_buffers(kc, ac, fill)
        L.check(ctx.lib.ov2_lckf_prepare(ctx.h, im.ctypes.data_as(C.c_void_p), im.shape[1], im.shape[0], im.strides[0], C.byref(p),
                                         e.ctypes.data_as(C.c_void_p) if len(e) else None, len(e), C.byref(r)))
        return [(r, out)]
    return _lckf_retry(call, want_all, kept_cap, all_cap, raw)[0]


def lckf_prepare_tracker(tracker, params, excl_xy, want_all=False, kept_cap=None, all_cap=None):
    """ov2_tracker_lckf_prepare: the same on the raw frame a VisualFrontEndTracker holds on the device (no image upload)"""
    e, p = _excl(excl_xy), _as_lckf_params(params)

    def call(kc, ac):
        r, out = lckf_buffers(kc, ac)
        L.check(tracker.lib.ov2_tracker_lckf_prepare(tracker.h_trk, C.byref(p), e.ctypes.data_as(C.c_void_p) if len(e) else None, len(e),
                                                     C.byref(r)))
        return [(r, out)]
    return _lckf_retry(call, want_all, kept_cap, all_cap)[0]


def _excl_slots(excl_list):
    es = [_excl(e) for e in excl_list]
    cap = max([len(e) for e in es] + [0])
    slots = np.zeros((max(1, len(es)), max(1, cap), 2), np.float32)
    for b, e in enumerate(es):
        slots[b, :len(e)] = e
    return slots, np.array([len(e) for e in es], np.int32), cap


def lckf_prepare_btracker(btracker, params, excl_list, want_all=False, kept_cap=None, all_cap=None):
    """ov2_btracker_lckf_prepare: items [0, len(excl_list)) of the lock-step tracker's current step; one dict per item"""
    p = _as_lckf_params(params)
    slots, n, cap = _excl_slots(excl_list)
    if cap == 0:
        slots = slots[:, :0]

    def call(kc, ac):
        R = (L.LckfResult * len(n))()
        outs = []
        for b in range(len(n)):
            R[b], out = lckf_buffers(kc, ac)
            outs.append(out)
        L.check(btracker.lib.ov2_btracker_lckf_prepare(btracker.h_trk, len(n), C.byref(p), slots.ctypes.data_as(C.c_void_p) if cap else None,
                                                       n.ctypes.data_as(C.c_void_p), cap, R))
        return [(R[b], outs[b]) for b in range(len(n))]
    return _lckf_retry(call, want_all, kept_cap, all_cap)


class _DeviceArrays:
    """device copies of numpy arrays through the HIP runtime the library is linked against (hipMalloc / hipMemcpy / hipFree)"""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.bufs = []

    def _ok(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed with HIP error %d" % (what, rc))

    def upload(self, a):
        p = C.c_void_p()
        self._ok(self.hip.hipMalloc(C.byref(p), max(a.nbytes, 1)), "hipMalloc")
        self.bufs.append(p)
        if a.nbytes:
            self._ok(self.hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1), "hipMemcpy")
        return p.value

    def download(self, ptr, a):
        if a.nbytes:
            self._ok(self.hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), a.nbytes, 2), "hipMemcpy")
        return a

    def free(self):
        for p in self.bufs:
            self.hip.hipFree(p)
        self.bufs = []


def lckf_prepare_batch(ctx, params, imgs, excl_list, want_all=False, kept_cap=None, all_cap=None, fill=0):
    """ov2_lckf_prepare_batch_d on a stack of equally sized host images (n, h, w): the stack and the exclusion lists are copied to
    the device, the lists come back as one dict per item (each with "raw": the whole slot arrays, pre-set to `fill`).  A caller
    whose frames are resident calls lckf_prepare_batch_d with addresses instead."""
    p = _as_lckf_params(params)
    st = np.ascontiguousarray(imgs, dtype=np.uint8)
    if st.ndim != 3 or len(excl_list) != len(st):
        raise ValueError("lckf_prepare_batch: imgs must be (n, h, w) with one exclusion list per image")
    B, h, w = st.shape
    if B == 0:
        return []
    slots, n, cap = _excl_slots(excl_list)
    dev = _DeviceArrays()
    try:
        d_img, d_ex, d_n = dev.upload(st), dev.upload(slots), dev.upload(n)

        def call(kc, ac):
            hst = dict(kept_xy=np.full((B, kc, 2), fill, np.int16), kept_resp=np.full((B, kc), fill, np.uint8),
                       kept_valid=np.full((B, kc), fill, np.uint8), kept_desc=np.full((B, kc, L.OV2_BRIEF_BYTES), fill, np.uint8),
                       all_xy=np.full((B, ac, 2), fill, np.int16), all_resp=np.full((B, ac), fill, np.uint8), counts=np.zeros((B, 4), np.int32))
            for a in hst.values():
                a.view(np.uint8)[...] = fill
            d = {k: dev.upload(v) for k, v in hst.items()}
            lckf_prepare_batch_d(ctx, p, d_img, w, h, w, w * h, B, d_ex if cap else 0, cap, d_n if cap else 0,
                                 d["all_xy"] if ac else 0, d["all_resp"] if ac else 0, ac, d["kept_xy"] if kc else 0, d["kept_resp"] if kc else 0,
                                 d["kept_valid"] if kc else 0, d["kept_desc"] if kc else 0, kc, d["counts"])
            for k, v in hst.items():
                dev.download(d[k], v)
            rs = []
            for b in range(B):
                r = L.LckfResult()
                r.n_all, r.cut, r.n_kept, r.n_desc = (int(v) for v in hst["counts"][b])
                r.kept_cap, r.all_cap = kc, ac
                rs.append((r, {k: hst[k][b] for k in hst if k != "counts"}))
            return rs
        return _lckf_retry(call, want_all, kept_cap, all_cap, raw=True)
    finally:
        dev.free()


def lckf_prepare_batch_d(ctx, params, img_d, w, h, pitch, item_stride, n_items, excl_xy_d, excl_cap, n_excl_d, all_xy_d, all_resp_d, all_cap,
                         kept_xy_d, kept_resp_d, kept_valid_d, kept_desc_d, kept_cap, counts_d):
    """ov2_lckf_prepare_batch_d: every array argument a device address (int; 0 = NULL)"""
    v = lambda a: C.c_void_p(int(a)) if a else None
    L.check(ctx.lib.ov2_lckf_prepare_batch_d(ctx.h, C.byref(_as_lckf_params(params)), v(img_d), int(w), int(h), int(pitch), int(item_stride),
                                             int(n_items), v(excl_xy_d), int(excl_cap), v(n_excl_d), v(all_xy_d), v(all_resp_d), int(all_cap),
                                             v(kept_xy_d), v(kept_resp_d), v(kept_valid_d), v(kept_desc_d), int(kept_cap), v(counts_d)))


# ---- local-map tracking of a loop candidate (the plumbing is _mapmatch's, shared with mapper.py) ------------------------------------
LOOPMAP_BEHIND, LOOPMAP_OUT_OF_FOV, LOOPMAP_OUT_OF_IMAGE = L.OV2_LOOPMAP_BEHIND, L.OV2_LOOPMAP_OUT_OF_FOV, L.OV2_LOOPMAP_OUT_OF_IMAGE
LOOPMAP_NO_CANDIDATE, LOOPMAP_RATIO_REJECTED, LOOPMAP_BEST = L.OV2_LOOPMAP_NO_CANDIDATE, L.OV2_LOOPMAP_RATIO_REJECTED, L.OV2_LOOPMAP_BEST

_LOOPMAP_FIELDS = (("kp_px", np.float32, C.c_float), ("kp_mp", np.int32, C.c_int), ("kp_matched", np.uint8, C.c_uint8),
                   ("cell_start", np.int32, C.c_int), ("cell_kp", np.int32, C.c_int), ("obs_start", np.int32, C.c_int),
                   ("obs_kfid", np.int32, C.c_int), ("desc_start", np.int32, C.c_int), ("desc", np.uint8, C.c_uint8),
                   ("lm_mp", np.int32, C.c_int), ("lm_wpt", np.float64, C.c_double))
_LOOPMAP = _mapmatch.Family("loop_match_to_map", "ov2_loop_match_to_map", "ov2_loop_match_to_map_batch", L.LoopMapParams, L.LoopMapItem,
                            L.LoopMapResult, _LOOPMAP_FIELDS, defaults=dict(fmax_proj_pxdist=10.0))


def loopmap_params(K, D, *, model="pinhole", img_w, img_h, ncellsize, fmax_proj_pxdist=10.0, fmax_desc_dist, desc_bytes=32):
    """ov2_loopmap_params: the left camera's model / K (fx fy cx cy) / distortion vector (None or empty: none) / image size, the
    Frame's ncellsize_, and maxdist / ratio as LoopCloser::processLoopCandidate passes them (10. and fmax_desc_dist_ * 1.5).
    The returned struct keeps its distortion array alive."""
    return _LOOPMAP.params(K, D, model, img_w, img_h, ncellsize, fmax_proj_pxdist, fmax_desc_dist, desc_bytes)


_as_loopmap_params = _LOOPMAP.as_params
_loopmap_item = _LOOPMAP.item        # (ov2_loopmap_item, the arrays it points into, n_lm, n_kp)
_loopmap_result = _LOOPMAP.result    # (ov2_loopmap_result, the dict of arrays it points into)


def loop_match_to_map(ctx, params, item):
    """ov2_loop_match_to_map: LoopCloser::matchToMap for one loop candidate.  Returns the result arrays as a dict (module docstring)."""
    return _LOOPMAP.call(ctx, params, item)


def loop_match_to_map_batch(ctx, params, items):
    """ov2_loop_match_to_map_batch: several candidates in one call (shared params).  Returns one dict per item, as loop_match_to_map."""
    return _LOOPMAP.call_batch(ctx, params, items)
