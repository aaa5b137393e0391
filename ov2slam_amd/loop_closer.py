"""Host-side mirror of the loop closer's descriptor matching (the reference's LoopCloser::knnMatching, src/loop_closer.cpp:378-459)
on top of the C ABI (ov2_knn_match[_batch], csrc/knn.hip): a brute-force Hamming 2-nearest-neighbour search of every query
descriptor among the train descriptors, the distance gate and the ratio test.

An item is a pair (query, train) of uint8 arrays of shape (n, 32); either may be empty.  A result is a dict: idx (n_query, 2) int32
(train rows of the nearest and the second nearest, -1: none), dist (n_query, 2) int32 (their Hamming distances, -1 where idx is -1),
good (n_query,) uint8, pairs (n_pairs, 2) int32 (query row, train row) of the good rows in query order.  The two frame walks that
collect the rows and their ids (:391-420) stay with the caller, who maps the pairs through vkpids / vlmids."""
import ctypes as C

import numpy as np

from . import _lib as L


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
