"""Grid-detector scenes (plain numpy + the CPU oracle) that walk detectSingleScale / detectGridFAST through every launch geometry
and in-kernel branch that csrc/detect.hip derives from the cell size: what tests/test_detect_cases.py checks on the oracle alone and
tests/test_gpu_detect_cases.py runs through the HIP kernels.

A scene is a dict: image, cell, current keypoints, ROI, starting quality, starting FAST threshold.
  * sizes: 264 x 200 (width no multiple of 32: the last mask word of a row is partial; 33 x 25 cells at cell 8, 4 x 3 at cell 64) and
    193 x 131,
  * contents: the synth texture, uniform noise (near-ties), the texture with a constant left half (all-zero responses: the arg-max is the
    first pixel and fails the gate), a flat frame, and three noise rows repeated down the image (inside a cell the responses of rows y and
    y + 3 are equal to the bit: several maxima in one column, of which the first in raster order has to win),
  * current keypoints: none / a third of the cells / every cell / more than 1024 / "mixed" = a third of the cells plus points that hug the border of
    their cell (the exclusion disc reaches into free neighbours), points exactly on cell boundaries, at .5 coordinates, outside the image
    on every side, in the partial strip right of and below the last full cell, and a duplicate -- permuted; "edge" = the outside and partial-strip points alone; "occupy:k" =
    exactly k cells, which sets the number of free cells against the strip kernel's cells per work-group,
  * ROIs: the usual (5, 5, w - 10, h - 10) and one that cuts through cells,
  * border shapes on both sides of the in-image test x0 + cell < w - 1.
Scenes and the oracle's answers on them are cached: computed once per process, shared and never modified."""
import functools

import numpy as np

from ov2slam_amd import synth

MAIN, ODD = (264, 200), (193, 131)
CELLS = tuple(range(8, 65))
CONTENTS = ("texture", "noise", "halfconst", "flat", "periodic")
Q_MID, Q_ALL = 2e-2, 10.0            # starting qualities beside 1e-3: one that rejects a good share of the cells, one that rejects all
MASK_AS_EXECUTED, MASK_INTENDED = 0, 1
TIE_SCAN_ORDER, TIE_LIBSTDCXX = 0, 1
BORDER_CELLS = (8, 36, 37, 52, 53, 64)
SOBEL_CELLS = (8, 17, 37, 52, 63)
BATCH_CELLS = (8, 36, 37, 52, 53, 63, 64)
BATCH_ITEMS = 70


STRIP_STATIC_LDS = 432              # k_mineig_strip's static LDS in the gfx950 build (tests/test_detect_cases.py reads it from a device-only compile)


def strip_lds(cell, k):
    return ((cell * 64 * k + 15) & ~15) + k * cell * 65 * 4


def strip_geometry(cell, static_lds=STRIP_STATIC_LDS):
    """(cells per work-group, wavefronts per work-group) of k_mineig_strip: the packing that leaves the fewest lanes idle when a
    wavefront owns at most 60 of its 64 columns, among those whose dynamic plus static LDS fits 160 KB.  A statement about the test inputs
    (which free-cell counts fill the last work-group and which do not), not a copy of the kernel.  Only cells 63 and 64 come near the
    limit (7 cells on 8 wavefronts: 163296 and 165888 B): any static size up to 544 B gives the same answer."""
    lds_limit = 160 * 1024 - static_lds
    best = None
    for nc in range(1, 9):
        k = (nc * cell + 59) // 60
        if k > 8:
            break
        if strip_lds(cell, k) > lds_limit:
            continue
        e = nc * cell / (64.0 * k)
        if best is None or e > best[0] + 1e-9:
            best = (e, nc, k)
    return best[1], best[2]


def select_instance(mode, cell, items=1):
    """the k_grid_select<MODE, MAXROW, CHUNKS, NT> instance enqueue_detect picks"""
    mr, ch = (36, 1) if cell <= 36 else ((52, 1) if cell <= 52 else (32, 2))
    return (mode, mr, ch, 512 if items >= 64 else 1024)


@functools.lru_cache(maxsize=None)
def image(content, w, h, seed=0):
    rng = np.random.default_rng(1000 + seed)
    if content == "noise":
        img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    elif content == "flat":
        img = np.full((h, w), 128, np.uint8)
    elif content == "periodic":                                     # three noise rows repeated: equal responses three rows apart
        img = np.ascontiguousarray(np.tile(rng.integers(0, 256, (3, w), dtype=np.uint8), (-(-h // 3), 1))[:h])
    else:
        tex, _, _ = synth.frame_pair(MAIN[0], MAIN[1], seed=31 + seed)
        reps = (-(-h // MAIN[1]), -(-w // MAIN[0]))
        img = np.ascontiguousarray(np.tile(tex, reps)[:h, :w])
        if content == "halfconst":
            img = img.copy(); img[:, :w // 2] = 93
    img.setflags(write=False)
    return img


def usual_roi(w, h):
    return (5, 5, w - 10, h - 10)                                   # camera_calibration.cpp:72-73


def cut_roi(w, h):
    return (37, 29, w - 80, h - 61)                                 # cuts through cells: primaries are rejected, and their secondaries


def mixed_keypoints(w, h, cell, rng, edge_only=False):
    nw, nh = w // cell, h // cell
    if nw == 0 or nh == 0:
        return np.array([[w / 2, h / 2], [-3.0, 2.0]], np.float32)
    if edge_only:                                                   # (images of a few cells: the full list would occupy them all)
        pts = [np.array([[-3.5, 10.0], [-20.0, -20.0], [w + 5.0, 50.0], [40.0, h + 7.0], [w - 0.4, h - 0.4], [w - 2.5, -1.0],
                         [w + 2.0 * cell, h + 2.0 * cell], [nw * float(cell), h - 1.5]])]
        if nw * cell < w:
            pts.append(np.stack([rng.uniform(nw * cell, w - 0.5, 2), rng.uniform(0, h - 1, 2)], 1))
        if nh * cell < h:
            pts.append(np.stack([rng.uniform(0, w - 1, 2), rng.uniform(nh * cell, h - 0.5, 2)], 1))
        p = np.concatenate(pts)
        return np.ascontiguousarray(p[rng.permutation(len(p))], np.float32)
    grid = synth.grid_keypoints(w, h, cell, rng).astype(np.float64)
    pts = [grid[::3]]
    # border huggers: in every third cell (the occupied ones) a point within cell / 4 of the cell's border
    hug = []
    for i in range(0, nw * nh, 3):
        r, c = divmod(i, nw)
        d, t = rng.uniform(0, cell / 4.0), rng.uniform(0, cell - 0.01)
        side = int(rng.integers(4))
        x, y = [(d, t), (cell - 0.01 - d, t), (t, d), (t, cell - 0.01 - d)][side]
        hug.append((c * cell + max(0.0, x), r * cell + max(0.0, y)))
    pts.append(np.array(hug))
    # exactly on cell boundaries, x and y
    kx, ky = rng.integers(0, nw + 1, 3), rng.integers(0, nh + 1, 3)
    pts.append(np.stack([kx * float(cell), rng.uniform(0, h - 1, 3)], 1))
    pts.append(np.stack([rng.uniform(0, w - 1, 3), ky * float(cell)], 1))
    # .5 coordinates: the disc centre rounds half to even
    pts.append(np.floor(np.stack([rng.uniform(1, w - 2, 4), rng.uniform(1, h - 2, 4)], 1)) + 0.5)
    # outside the image on every side; the disc of some reaches in
    pts.append(np.array([[-3.5, 10.0], [-20.0, -20.0], [w + 5.0, 50.0], [40.0, h + 7.0], [w - 0.4, h - 0.4], [30.0, -1.0], [-0.6, h / 2.0],
                         [w + 2.0 * cell, h + 2.0 * cell]]))
    # the partial strip right of and below the last full cell
    if nw * cell < w:
        pts.append(np.stack([rng.uniform(nw * cell, w - 0.5, 2), rng.uniform(0, h - 1, 2)], 1))
    if nh * cell < h:
        pts.append(np.stack([rng.uniform(0, w - 1, 2), rng.uniform(nh * cell, h - 0.5, 2)], 1))
    p = np.concatenate(pts)
    p = np.concatenate([p, p[1:2]])                                 # a duplicated point
    return np.ascontiguousarray(p[rng.permutation(len(p))], np.float32)


def keypoints(kind, w, h, cell, seed):
    rng = np.random.default_rng(7000 + 97 * cell + seed)
    nw, nh = w // cell, h // cell
    if kind == "none" or nw * nh == 0 and kind != "mixed":
        return np.zeros((0, 2), np.float32)
    if kind == "third":
        return synth.grid_keypoints(w, h, cell, rng)[::3]
    if kind == "all":
        return synth.grid_keypoints(w, h, cell, rng, jitter=0.3)
    if kind == "mixed":
        return mixed_keypoints(w, h, cell, rng)
    if kind == "edge":
        return mixed_keypoints(w, h, cell, rng, edge_only=True)
    if kind == "many":                                              # more than 1024 points
        return np.stack([rng.uniform(-4, w + 4, 1500), rng.uniform(-4, h + 4, 1500)], 1).astype(np.float32)
    if kind.startswith("occupy:"):                                  # exactly k cells, evenly spread, at their centres
        k = int(kind.split(":")[1])
        idx = np.arange(k) * ((nw * nh) // k)
        return np.stack([(idx % nw + 0.5) * cell, (idx // nw + 0.5) * cell], 1).astype(np.float32)
    raise ValueError(kind)


def scene(content, cell, kind, roi="usual", quality=1e-3, fast_th=10, size=MAIN, seed=0):
    return _scene(content, int(cell), kind, roi, float(quality), int(fast_th), tuple(size), int(seed))


@functools.lru_cache(maxsize=None)
def _scene(content, cell, kind, roi, quality, fast_th, size, seed):
    w, h = size
    cur = keypoints(kind, w, h, cell, seed)
    cur.setflags(write=False)
    return dict(name="%s/%d/%s/%s/q%g/th%d/%dx%d/s%d" % (content, cell, kind, roi, quality, fast_th, w, h, seed), content=content, img=image(content, w, h, seed),
                w=w, h=h, cell=cell, kind=kind, cur=cur, roi=usual_roi(w, h) if roi == "usual" else cut_roi(w, h), quality=quality, fast_th=fast_th)


def occupy_counts(cell, size=MAIN):
    """numbers of occupied cells that leave a free-cell count that is / is not a multiple of the strip kernel's cells per work-group
    (the second is None where that is 1 cell: every count is a multiple)"""
    ncells = (size[0] // cell) * (size[1] // cell)
    n, _ = strip_geometry(cell)
    mult = next(k for k in range(1, ncells) if (ncells - k) % n == 0)
    non = next((k for k in range(1, ncells) if (ncells - k) % n != 0), None)
    return mult, non


@functools.lru_cache(maxsize=None)
def sweep(cell):
    """the scenes of one cell size on the main shape: every content, every keypoint kind, both ROIs, the three qualities and thresholds"""
    mult, non = occupy_counts(cell)
    s = [scene("texture", cell, "mixed", "usual", 1e-3, 10),
         scene("texture", cell, "none", "cut", Q_MID, 5),
         scene("texture", cell, "all", "usual", 1e-3, 40),
         scene("noise", cell, "third", "usual", 1e-3, 5),
         scene("noise", cell, "mixed", "cut", 1e-3, 10, seed=1),
         scene("halfconst", cell, "occupy:%d" % mult, "usual", 1e-3, 10),
         scene("halfconst", cell, "mixed", "usual", Q_ALL, 40, seed=2),
         scene("flat", cell, "none", "usual", 1e-3, 10),
         scene("periodic", cell, "third", "usual", 1e-3, 10, seed=7),
         scene("periodic", cell, "none", "usual", 1e-3, 5, seed=9)]
    if non is not None:
        s.append(scene("texture", cell, "occupy:%d" % non, "usual", Q_MID, 10, seed=3))
    if cell == 8:
        s.append(scene("texture", cell, "many", "usual", 1e-3, 10, seed=4))
    # a shape with a last column of cells that fails the in-image test (n cell + 1 wide), whatever the main shape does at this cell
    s.append(scene("noise", cell, "third", "usual", 1e-3, 10, size=(max(3, 96 // cell) * cell + 1, max(2, 64 // cell) * cell + 3), seed=6))
    if cell % 8 == 1:                                               # the odd shape now and then: another mask pitch, other cell counts
        s.append(scene("texture", cell, "mixed", "usual", 1e-3, 10, size=ODD, seed=5))
    return tuple(s)


@functools.lru_cache(maxsize=None)
def border_scenes(cell):
    """widths and heights n cell, n cell + 1, n cell + 2 and (n + 1) cell - 1 (both sides of x0 + cell < w - 1), one cell row, one cell
    column, and an image smaller than one cell"""
    nx, ny = (5, 4) if cell <= 16 else ((3, 2) if cell <= 40 else (2, 2))
    ws = [nx * cell, nx * cell + 1, nx * cell + 2, (nx + 1) * cell - 1]
    hs = [ny * cell, ny * cell + 1, ny * cell + 2, (ny + 1) * cell - 1]
    sizes = [(ws[i], hs[(i + j) % 4]) for i in range(4) for j in (0, 1)]                   # every width and every height, twice; (ws[2], hs[2]) among them
    sizes += [(3 * cell + 2, cell + 2 + (cell - 3) // 2), (cell + 2 + (cell - 3) // 2, 3 * cell + 2)]     # one cell row, one cell column
    sizes += [(cell - 1, cell + 5), (cell + 5, cell - 1)]                                  # smaller than one cell: empty
    out = []
    for i, (w, h) in enumerate(sizes):
        inside = (w, h) == (ws[2], hs[2])                          # every cell passes the in-image test: noise, no keypoints and a low
        content = "noise" if i % 2 or inside else "texture"        # quality give every cell a primary, so no secondary list is written
        q = 1e-6 if inside else 1e-3
        kind = "none" if inside or i % 3 == 0 else ("mixed" if (w // cell) * (h // cell) >= 12 and i % 3 == 1 else "edge")
        out.append(_scene(content, cell, kind, "usual", q, 10 if i % 2 else 5, (w, h), 10 + i))
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------------ oracle runs
@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import oracle as O
    O.build()
    return O


def _key(s):
    return s["name"]                                                # (names are unique: every parameter of the scene is in them)


_CACHE = {}


def _cached(key, fn):
    if key not in _CACHE:
        pts, state = fn()
        pts.setflags(write=False)
        _CACHE[key] = (pts, state)
    return _CACHE[key]


def oracle_singlescale(s, subpix, sobel_dy=0):
    O = _oracle()

    def run():
        prev = O.set_sobel_dy_order(sobel_dy)
        try:
            return O.detect_singlescale(s["img"], s["cell"], s["cur"], s["roi"], s["quality"], subpix=subpix)
        finally:
            O.set_sobel_dy_order(prev)
    return _cached(("ss", _key(s), bool(subpix), sobel_dy), run)


def oracle_fast(s, mask_mode, tie, subpix=False, fast_th=None):
    O = _oracle()
    th = s["fast_th"] if fast_th is None else fast_th

    def run():
        with O.fast_tie_mode(tie):
            return O.detect_grid_fast(s["img"], s["cell"], s["cur"], th, mask_mode, subpix=subpix)
    return _cached(("fast", _key(s), mask_mode, tie, bool(subpix), th), run)


# ------------------------------------------------------------------------------------------------------------------ branch counts
def occupancy(s):
    """voccupcells as the reference fills it: float division, truncation"""
    cell, nw, nh = s["cell"], s["w"] // s["cell"], s["h"] // s["cell"]
    occ = np.zeros((nh + 1, nw + 1), bool)
    for px, py in s["cur"]:
        r, c = int(np.float32(py) / np.float32(cell)), int(np.float32(px) / np.float32(cell))
        if 0 <= r <= nh and 0 <= c <= nw:
            occ[r, c] = True
    return occ[:nh, :nw]


def start_mask(s):
    O = _oracle()
    mask = np.ones((s["h"], s["w"]), np.uint8)
    for px, py in s["cur"]:
        O.circle_fill0(mask, int(np.rint(np.float32(px))), int(np.rint(np.float32(py))), s["cell"] // 4)
    return mask


def trace_singlescale(s):
    """detectSingleScale's selection restated cell by cell on oracle.cell_mineig and oracle.circle_fill0, to count the branches; returns
    (points, counts).  tests/test_detect_cases.py asserts that the points are oracle.detect_singlescale's."""
    O = _oracle()
    cell, w, h = s["cell"], s["w"], s["h"]
    nw, nh = w // cell, h // cell
    k = dict(cells=nw * nh, occupied=0, skipped=0, primaries=0, secondaries=0, sec_written=0, sec_absent=0, sec_truncated=0, roi_rejected=0,
             q_rejected=0, mask_decided=0, zero_cells=0, sec_absent_full=0, column_ties=0)
    if nw * nh == 0:
        return np.zeros((0, 2), np.float32), k
    occ, mask = occupancy(s), start_mask(s)
    rx, ry, rw, rh = s["roi"]
    q, R = s["quality"], cell // 4
    prim, sec = [], []

    def masked_argmax(hm, x0, y0):
        v = hm * mask[y0:y0 + cell, x0:x0 + cell].astype(np.float32)
        i = int(np.argmax(v))                                       # first maximum in raster order
        return float(v.flat[i]), x0 + i % cell, y0 + i // cell

    for r in range(nh):
        for c in range(nw):
            if occ[r, c]:
                k["occupied"] += 1; continue
            x0, y0 = c * cell, r * cell
            if not (x0 + cell < w - 1 and y0 + cell < h - 1):
                k["skipped"] += 1; continue
            hm = O.cell_mineig(s["img"], x0, y0, cell)
            plain = int(np.argmax(hm))
            k["zero_cells"] += int(not hm.any())
            first = None
            d, mx, my = masked_argmax(hm, x0, y0)
            # an accepted primary whose column holds its value more than once: the first of them in raster order wins
            k["column_ties"] += int(d >= q and d > 0 and (hm[:, mx - x0] == np.float32(d)).sum() > 1 and rx <= mx < rx + rw and ry <= my < ry + rh)
            if mx < rx or my < ry or mx >= rx + rw or my >= ry + rh:
                k["roi_rejected"] += 1; continue
            if d >= q:
                prim.append((mx, my)); first = (mx, my)
                O.circle_fill0(mask, mx, my, R)
            else:
                k["q_rejected"] += 1
            d, mx, my = masked_argmax(hm, x0, y0)
            if mx < rx or my < ry or mx >= rx + rw or my >= ry + rh:
                k["roi_rejected"] += 1
            elif d >= q:
                sec.append((mx, my)); first = first or (mx, my)
                O.circle_fill0(mask, mx, my, R)
            if first is not None and (first[0] - x0) + (first[1] - y0) * cell != plain:
                k["mask_decided"] += 1
    k["primaries"], k["secondaries"] = len(prim), len(sec)
    k["sec_absent_full"] = int(len(prim) > 0 and len(prim) + k["occupied"] == nw * nh)      # (not merely: every cell occupied)
    out = list(prim)
    if len(prim) + k["occupied"] < nw * nh:
        nbsec = nw * nh - (len(prim) + k["occupied"])
        out += sec[:nbsec]
        k["sec_written"] = min(len(sec), nbsec)
        k["sec_truncated"] = int(len(sec) > nbsec)
    else:
        k["sec_absent"] = 1
    return np.array(out, np.float32).reshape(-1, 2), k


def trace_fast(s, mask_mode):
    """detectGridFAST's selection restated on oracle.fast9_16, first maximum in scan order; returns (points, counts)"""
    O = _oracle()
    cell, w, h, th = s["cell"], s["w"], s["h"], s["fast_th"]
    nw, nh = w // cell, h // cell
    k = dict(cells=nw * nh, occupied=0, empty=0, skipped=0, points=0, sort_cells=0, tie_cells=0, weak=0)
    if nw * nh == 0:
        return np.zeros((0, 2), np.float32), k
    occ, mask = occupancy(s), start_mask(s)
    out = []
    for r in range(nh):
        for c in range(nw):
            if occ[r, c]:
                k["occupied"] += 1; continue
            k["empty"] += 1
            x0, y0 = c * cell, r * cell
            if not (x0 + cell < w - 1 and y0 + cell < h - 1):
                k["skipped"] += 1; continue
            xs, ys, sc = O.fast9_16(np.ascontiguousarray(s["img"][y0:y0 + cell, x0:x0 + cell]), th, True)
            if mask_mode == MASK_AS_EXECUTED:
                keep = ((xs & 3) >= 2) & (mask[y0 + ys, x0 + (xs >> 2)] != 0)
            else:
                keep = mask[y0 + ys, x0 + xs] != 0
            if not keep.any():
                continue
            ks = np.where(keep, sc, -1)
            b = int(np.argmax(ks))
            if keep.sum() > 16:
                k["sort_cells"] += 1
                k["tie_cells"] += int((ks == ks[b]).sum() > 1)
            if ks[b] >= 20:
                px, py = int(xs[b]) + x0, int(ys[b]) + y0
                O.circle_fill0(mask, px, py, cell // 4)
                out.append((px, py))
            else:
                k["weak"] += 1
    k["points"] = len(out)
    return np.array(out, np.float32).reshape(-1, 2), k


# ------------------------------------------------------------------------------------------------------------------ batches
@functools.lru_cache(maxsize=None)
def batch(cell):
    """70 items of 264 x 200 cycling through five images; per-item keypoint counts cycle through 0, a few, a third of the cells and all
    cells; per-item qualities and thresholds differ.  Returns (images (5), item -> image index, cur (B, cap, 2), ncur (B), q (B), th (B))."""
    w, h = MAIN
    ncells = (w // cell) * (h // cell)
    imgs = [image("texture", w, h, 0), image("noise", w, h, 1), image("halfconst", w, h, 2), image("flat", w, h, 0), image("texture", w, h, 3)]
    B = BATCH_ITEMS
    which = np.arange(B) % 5
    cap = ncells + 8
    cur = np.full((B, cap, 2), np.nan, np.float32)                  # unused slots hold NaN: nothing may read them
    ncur = np.zeros(B, np.int32)
    for b in range(B):
        rng = np.random.default_rng(500 + b)
        kind = b % 4
        if kind == 1:
            p = mixed_keypoints(w, h, cell, rng)[:min(5, cap)]
        elif kind == 2:
            p = synth.grid_keypoints(w, h, cell, rng)[::3]
        elif kind == 3:
            p = synth.grid_keypoints(w, h, cell, rng, jitter=0.3)
        else:
            p = np.zeros((0, 2), np.float32)
        cur[b, :len(p)] = p; ncur[b] = len(p)
    q = np.array([1e-3, 1e-2, 1e-4, Q_MID, 0.5, 1e-3, Q_ALL][:7] * 10, np.float64)[:B]
    th = np.array([10, 20, 5, 10, 40, 7, 60, 3, 10] * 8, np.int32)[:B]
    return imgs, which, cur, ncur, q, th


def batch_item_scene(cell, b):
    imgs, which, cur, ncur, q, th = batch(cell)
    w, h = MAIN
    c = np.ascontiguousarray(cur[b, :ncur[b]])
    return dict(name="batch/%d/%d" % (cell, b), content="batch%d" % which[b], img=imgs[which[b]], w=w, h=h, cell=cell, kind="item%d" % b, cur=c,
                roi=usual_roi(w, h), quality=float(q[b]), fast_th=int(th[b]))
