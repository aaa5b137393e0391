"""Numpy specification of the loop closer's descriptor matching (the reference's LoopCloser::knnMatching, src/loop_closer.cpp:378-459),
written twice, as tests/match_ref.py is:

  replay(query, train, max_dist, ratio)   transcribes the path the reference takes through OpenCV.
      cv::BFMatcher(cv::NORM_HAMMING).knnMatch(query, train, vmatches, 2) ends in cv::batchDistance with K = 2: per query row the
      distances start at INT_MAX and the indices at -1; the train rows are visited in ascending order; a distance d is inserted only
      if d < dist[K-1], shifting entries down while dist[k] > d.  Both comparisons are strict, so among equal distances the lower
      train row comes first.  knnMatchImpl then emits, per query, the entries with index >= 0 as DMatch (distance as a float).
      Then the reference's loop :432-449: good if m.size() < 2, otherwise good if d0 <= maxdist && d0 <= d1 * 0.85 (float times
      double: the product in double); a good row appends (queryIdx, trainIdx) of m[0].
  flat(query, train, max_dist, ratio)     states the same order-free: the two neighbours of a query row are the two smallest
      (distance, train row) pairs in lexicographic order.  This is the form the GPU tests compare against, and what makes any
      split of the train rows with a merge legal.

Both return a dict: idx (n_q, 2) int32 (train row or -1), dist (n_q, 2) int32 (the Hamming distance, what DMatch::distance holds as
a float; -1 where idx is -1), good (n_q,) uint8, pairs (n_pairs, 2) int32 (query row, train row) of the good rows in query order.
Several queries may take the same train row: there is no cross-check, as in the reference.

BFMatcher::knnMatch is restated from OpenCV's published source, not pinned against an OpenCV build: there is none here.

Quirks kept:
  * a train set of ONE row makes EVERY query good whatever its distance (m.size() < 2), the distance gate included;
  * an empty query or train set yields no pairs (the reference returns at :422-424 before it matches); with an empty train set
    idx and dist are all -1 and good is 0;
  * (d0, d1) = (0, 0) passes the ratio test (two identical train rows equal to the query): 0 <= 0 * 0.85;
  * maxdist = int(cols * 0.5 * 8.) is 128 for 32 bytes, and the gate is d0 <= maxdist.
The ratio test is (double)d0 <= (double)d1 * ratio in fp64 without contraction.  For ratio = 0.85 and 0 <= d0 <= d1 <= 256 it equals
the exact 20 d0 <= 17 d1 (tests/test_knn_reference.py enumerates it), equalities (17, 20), (34, 40), ... (204, 240) included."""
import numpy as np

DESC_BYTES = 32
MAX_DIST = int(DESC_BYTES * 0.5 * 8.)      # :430
RATIO = 0.85
INT_MAX = 2 ** 31 - 1
FIELDS = ("idx", "dist", "good", "pairs")

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def _rows(a):
    a = np.ascontiguousarray(a, np.uint8)
    return a.reshape(0, DESC_BYTES) if a.size == 0 else a.reshape(-1, DESC_BYTES)


def hamming_matrix(query, train):
    """(n_q, n_t) int32 Hamming distances"""
    q, t = _rows(query), _rows(train)
    out = np.zeros((len(q), len(t)), np.int32)
    for i in range(0, len(q), 256):                                     # blocks: the xor cube stays small
        out[i:i + 256] = _POP[q[i:i + 256, None, :] ^ t[None, :, :]].sum(axis=2, dtype=np.int32)
    return out


def ratio_ok(d0, d1, ratio):
    """(double)d0 <= (double)d1 * ratio"""
    return bool(np.float64(d0) <= np.float64(d1) * np.float64(ratio))


def _pack(idx, dist, good):
    idx, dist, good = np.asarray(idx, np.int32).reshape(-1, 2), np.asarray(dist, np.int32).reshape(-1, 2), np.asarray(good, np.uint8)
    rows = np.nonzero(good)[0]
    pairs = np.stack([rows, idx[rows, 0]], axis=1).astype(np.int32).reshape(-1, 2)
    return dict(idx=idx, dist=dist, good=good, pairs=pairs)


def replay(query, train, max_dist=MAX_DIST, ratio=RATIO, ev=None):
    """the OpenCV path row by row; ev (a dict) collects what the campaign met"""
    q, t = _rows(query), _rows(train)
    n_q, n_t = len(q), len(t)
    idx, dist, good = np.full((n_q, 2), -1, np.int32), np.full((n_q, 2), -1, np.int32), np.zeros(n_q, np.uint8)
    if n_q == 0 or n_t == 0:                                            # :422-424
        return _pack(idx, dist, good)
    K = 2
    for i in range(n_q):
        bd, bi = [INT_MAX] * K, [-1] * K                                # batchDistance
        for j in range(n_t):
            d = int(_POP[q[i] ^ t[j]].sum())
            if d < bd[K - 1]:
                k = K - 2
                while k >= 0 and bd[k] > d:
                    bd[k + 1], bi[k + 1] = bd[k], bi[k]
                    k -= 1
                bd[k + 1], bi[k + 1] = d, j
            elif ev is not None and d == bd[K - 1] and bd[0] < d:       # a later row as close as the second: the earlier one stays
                ev["tie_second"] = ev.get("tie_second", 0) + 1
        m = [(np.float32(bd[k]), bi[k]) for k in range(K) if bi[k] >= 0]   # knnMatchImpl: DMatch(queryIdx, trainIdx, distance)
        if ev is not None and len(m) == 2 and m[0][0] == m[1][0]:
            ev["tie_first"] = ev.get("tie_first", 0) + 1
        for k, (d, j) in enumerate(m):
            idx[i, k], dist[i, k] = j, int(d)
        if len(m) < 2:                                                  # :435
            bgood, why = True, "good_single"
        elif not m[0][0] <= max_dist:                                   # :438, float against int
            bgood, why = False, "rej_dist"
        elif not np.float64(m[0][0]) <= np.float64(m[1][0]) * np.float64(ratio):      # :439, float * double
            bgood, why = False, "rej_ratio"
        else:
            bgood, why = True, "good_ratio"
            if ev is not None and 20 * int(m[0][0]) == 17 * int(m[1][0]) and ratio == RATIO and m[0][0] > 0:
                ev["ratio_equality"] = ev.get("ratio_equality", 0) + 1
        if ev is not None:
            ev[why] = ev.get(why, 0) + 1
        good[i] = bgood
    return _pack(idx, dist, good)


def flat(query, train, max_dist=MAX_DIST, ratio=RATIO):
    """order-free: the two smallest (distance, train row) per query row"""
    q, t = _rows(query), _rows(train)
    n_q, n_t = len(q), len(t)
    idx, dist, good = np.full((n_q, 2), -1, np.int32), np.full((n_q, 2), -1, np.int32), np.zeros(n_q, np.uint8)
    if n_q and n_t:
        H = hamming_matrix(q, t).astype(np.int64)
        key = H * (1 << 32) + np.arange(n_t, dtype=np.int64)[None, :]   # lexicographic (distance, row) as one integer
        k = min(2, n_t)
        best = np.sort(key, axis=1)[:, :k]
        idx[:, :k] = (best & 0xFFFFFFFF).astype(np.int32)
        dist[:, :k] = (best >> 32).astype(np.int32)
        if n_t == 1:
            good[:] = 1
        else:
            d0, d1 = dist[:, 0].astype(np.float64), dist[:, 1].astype(np.float64)
            good[:] = (dist[:, 0] <= max_dist) & (d0 <= d1 * np.float64(ratio))
    return _pack(idx, dist, good)


def same(a, b):
    """(equal, first differing field)"""
    for f in FIELDS:
        x, y = np.asarray(a[f]), np.asarray(b[f])
        if x.shape != y.shape or x.dtype != y.dtype or not np.array_equal(x, y):
            return False, f
    return True, None


# ---- generated cases ---------------------------------------------------------------------------------------------------------------
def flip(rng, row, nbits):
    """a copy of `row` with nbits distinct bits flipped: Hamming distance exactly nbits"""
    out = np.array(row, np.uint8)
    for b in rng.choice(8 * DESC_BYTES, size=int(nbits), replace=False):
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def make_case(rng, n_q, n_t, true_frac=0.5, twin_frac=0.3, dup_frac=0.1, gate_frac=0.1, max_dist=MAX_DIST):
    """(query, train): random descriptors alone never pass the ratio test (the distances cluster around 128), so the train set is
    planted with: true matches (a query row with a few bits flipped), ratio twins (a second train row at nearly the same distance
    from the same query), exact duplicates of a train row, and rows at distance exactly max_dist and max_dist + 1 from a query.
    Every planted row overwrites a random train row, so n_t is kept."""
    query = rng.integers(0, 256, (n_q, DESC_BYTES), dtype=np.uint8)
    train = rng.integers(0, 256, (n_t, DESC_BYTES), dtype=np.uint8)
    if n_q == 0 or n_t == 0:
        return query, train
    slots = list(rng.permutation(n_t))
    take = lambda: int(slots.pop()) if slots else int(rng.integers(n_t))
    budget = max(1, n_t // 2)                                           # plant into at most half of the train rows
    planted = 0
    for q in rng.permutation(n_q):
        if planted >= budget:
            break
        u = rng.uniform()
        if u < true_frac:
            k = int(rng.integers(0, 40))
            train[take()] = flip(rng, query[q], k); planted += 1
            v = rng.uniform()
            if v < twin_frac:                                           # a twin: the ratio test decides, equal distances included
                k2 = min(8 * DESC_BYTES, k + int(rng.integers(0, 12)))
                train[take()] = flip(rng, query[q], k2); planted += 1
            elif v < twin_frac + dup_frac:                              # an exact duplicate of the match: (k, k)
                a = take(); b = take()
                train[b] = train[a] = flip(rng, query[q], k); planted += 2
        elif u < true_frac + gate_frac:
            train[take()] = flip(rng, query[q], max_dist + int(rng.integers(0, 2))); planted += 1
    return query, train


# ---- crafted cases -----------------------------------------------------------------------------------------------------------------
def bits(k):
    """a descriptor with the k lowest bits set: at distance k from the all-zero query"""
    row = np.zeros(DESC_BYTES, np.uint8)
    row[:k // 8] = 0xFF
    if k % 8:
        row[k // 8] = (1 << (k % 8)) - 1
    return row


def _zq(n=1):
    return np.zeros((n, DESC_BYTES), np.uint8)


def _train(ks):
    return np.stack([bits(k) for k in ks]) if len(ks) else np.zeros((0, DESC_BYTES), np.uint8)


RATIO_EQUALITIES = [(17 * m, 20 * m) for m in range(1, 8)]             # d0 <= 128: (17, 20) ... (102, 120), (119, 140)


def crafted_cases(tile=256):
    """[(name, query, train, max_dist, ratio, good literal, idx literal)]: the query is all zeros (one row unless said), so a train
    row made by bits(k) is at distance exactly k.  `tile` is the kernel's train rows per LDS tile."""
    D, Rt = MAX_DIST, RATIO
    cases = []
    for d0, d1 in RATIO_EQUALITIES:
        cases.append(("ratio_eq_%d_%d" % (d0, d1), _zq(), _train([d1, d0]), D, Rt, [1], [[1, 0]]))
        cases.append(("ratio_above_%d_%d" % (d0 + 1, d1), _zq(), _train([d1, d0 + 1]), D, Rt, [0], [[1, 0]]))
    cases.append(("gate_128_151", _zq(), _train([128, 151]), D, Rt, [1], [[0, 1]]))
    cases.append(("gate_129_256", _zq(), _train([256, 129]), D, Rt, [0], [[1, 0]]))
    cases.append(("ratio_128_150", _zq(), _train([128, 150]), D, Rt, [0], [[0, 1]]))
    cases.append(("zero_zero", _zq(), _train([0, 0, 5]), D, Rt, [1], [[0, 1]]))
    cases.append(("three_tied", _zq(), _train([40, 40, 40, 90]), D, Rt, [0], [[0, 1]]))
    far = [200] * (tile + 3)
    far[0] = far[1] = far[tile + 1] = 40                                # the third of the tied rows sits in the next tile
    cases.append(("three_tied_across_tile", _zq(), _train(far), D, Rt, [0], [[0, 1]]))
    far = [200] * (2 * tile + 2)
    far[3] = 60; far[2 * tile + 1] = 30                                 # the best row comes after the second-best, two tiles later
    cases.append(("best_after_second", _zq(), _train(far), D, Rt, [1], [[2 * tile + 1, 3]]))
    cases.append(("best_after_second_adjacent", _zq(), _train([100, 70, 20]), D, Rt, [1], [[2, 1]]))
    cases.append(("single_train_row_256", _zq(3), _train([256]), D, Rt, [1, 1, 1], [[0, -1]] * 3))
    cases.append(("empty_query", _zq(0), _train([3, 4]), D, Rt, [], []))
    cases.append(("empty_train", _zq(2), _train([]), D, Rt, [0, 0], [[-1, -1]] * 2))
    return cases
