"""The keyframe rounds ov2_btracker_create_keyframe is tested on (plain numpy: no GPU, no library): what tests/test_createkf_cases.py
checks on the oracle alone and tests/test_gpu_createkf.py plays through the route (tests/createkf_ref.py) and the fused call.

Shapes: 376 x 240 frames without CLAHE (level 0 of the pyramid IS the frame), batch 4, 160 slots per item, a detection cell of 35 px
(10 x 6 cells: at most 120 new points with single scale, 60 with grid FAST) and the frame grid of 35 px cells (11 x 7), nbmaxkps 60.

A round is a dict: the frame it is played on, n_active, the params that differ from BASE, and one item spec per active item.  An item
spec names how its keypoints are made:
  empty      no keypoint (the tracker's first frame)
  few        40 keypoints in the top-left 110 x 75 px (at most 12 cells of the grid; some closer than 28 px to the border: invalid BRIEF)
  all        one keypoint in every cell of the frame grid (77 >= nbmaxkps: nothing to detect)
  crowd      150 keypoints in a 100 x 70 px patch (12 cells): the detector's top-up does not fit the 160 slots
  exact:k    k keypoints anywhere at least 30 px inside the image (the rounds that use it set nbmaxkps 0: nothing is detected, n_kf == k)
`order` is the order of the slot lmids (desc / random / asc), `dup` repeats one id, flag 0 leaves the item out of the request.
Rounds and scenes are built once per process, shared and never modified."""
import functools

import numpy as np

from ov2slam_amd import synth

W, H, BATCH, N_MAX, CELL = 376, 240, 4, 160, 35
BASE = dict(ncellsize=35, nbwcells=11, nbhcells=7, nbmaxkps=60, det_cell=CELL, roi=(5, 5, W - 10, H - 10), mask_mode=0, do_subpix=True,
            use_brief=True)
QUALITY0, FAST_TH0 = 1e-3, 20
NFRAMES = 3

ROUNDS = [
    dict(name="first", frame=0, n_active=4, twc="given",
         items=[dict(kind="empty"), dict(kind="empty"), dict(kind="empty"), dict(kind="empty")]),
    dict(name="mixed", frame=1, n_active=4, twc="given",
         items=[dict(kind="few", order="desc"), dict(kind="all", order="random"), dict(kind="few", order="asc", flag=0),
                dict(kind="crowd", order="random")]),
    dict(name="short", frame=1, n_active=3, twc="resident",
         items=[dict(kind="few", order="random", dup=True), dict(kind="all", order="asc", flag=0), dict(kind="few", order="asc")]),
    dict(name="sizes", frame=1, n_active=4, twc="given", params=dict(nbmaxkps=0, use_brief=False),
         items=[dict(kind="exact:1", order="asc"), dict(kind="exact:2", order="desc"), dict(kind="exact:64", order="random"),
                dict(kind="exact:65", order="random")]),
    dict(name="full", frame=1, n_active=4, twc="resident", params=dict(nbmaxkps=0),
         items=[dict(kind="exact:160", order="desc"), dict(kind="exact:128", order="asc"), dict(kind="exact:129", order="random"),
                dict(kind="empty")]),
    dict(name="last", frame=1, n_active=4, twc="resident",
         items=[dict(kind="few", order="random"), dict(kind="all", order="desc"), dict(kind="few", order="random", flag=0),
                dict(kind="few", order="desc")]),
]


def round_params(r, detector):
    p = dict(BASE, detector=detector)
    p.update(r.get("params", {}))
    return p


@functools.lru_cache(maxsize=None)
def frames():
    """frames()[b][f]: frame f of item b, and the flow between two frames of an item"""
    seqs = []
    for b in range(BATCH):
        rng = np.random.default_rng(90 + b)
        tex = synth.base_texture(max(W, H) + 500, 90 + b)
        views, offs = [], []
        ox, oy, th = 120.0, 110.0, 0.0
        for _ in range(NFRAMES):
            views.append(synth.warp(tex, W, H, ox, oy, th)); offs.append((ox, oy, th))
            ox += rng.uniform(-5, 5); oy += rng.uniform(-4, 4); th += rng.uniform(-0.006, 0.006)
        seqs.append((views, offs))
    return seqs


def flow(b, pts, f0, f1):
    """where the scene points seen at pts in frame f0 of item b lie in frame f1"""
    offs = frames()[b][1]
    (ox0, oy0, t0), (ox1, oy1, t1) = offs[f0], offs[f1]
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    dx, dy = pts[:, 0] - cx, pts[:, 1] - cy
    c, s = np.cos(t0), np.sin(t0)
    tx, ty = c * dx - s * dy + cx + ox0, s * dx + c * dy + cy + oy0
    dx, dy = tx - cx - ox1, ty - cy - oy1
    c, s = np.cos(-t1), np.sin(-t1)
    return np.stack([c * dx - s * dy + cx, s * dx + c * dy + cy], 1)


def _keypoints(kind, rng):
    if kind == "empty":
        return np.zeros((0, 2), np.float32)
    if kind == "few":
        return np.stack([rng.uniform(5, 110, 40), rng.uniform(5, 75, 40)], 1).astype(np.float32)
    if kind == "all":
        cs = BASE["ncellsize"]
        p = [(min(cs * c + rng.uniform(8, 27), W - 2), min(cs * r + rng.uniform(8, 27), H - 2))
             for r in range(BASE["nbhcells"]) for c in range(BASE["nbwcells"])]
        return np.array(p, np.float32)
    if kind == "crowd":
        return np.stack([rng.uniform(40, 140, 150), rng.uniform(40, 110, 150)], 1).astype(np.float32)
    k = int(kind.split(":")[1])
    return np.stack([rng.uniform(30, W - 30, k), rng.uniform(30, H - 30, k)], 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def round_inputs(ri):
    """the arrays of round ri in slot layout -> dict(px, lmid, is3d, n, make_kf, nlmid, nkfid, time, Twc (the poses given, also where the
    round takes the resident one))"""
    r = ROUNDS[ri]
    rng = np.random.default_rng(500 + ri)
    px = np.zeros((BATCH, N_MAX, 2), np.float32); lmid = np.zeros((BATCH, N_MAX), np.int32); is3d = np.zeros((BATCH, N_MAX), np.uint8)
    n = np.zeros(BATCH, np.int32); mk = np.zeros(BATCH, np.uint8); nlmid = np.zeros(BATCH, np.int32)
    for b, it in enumerate(r["items"]):
        p = _keypoints(it["kind"], rng)
        m = len(p)
        nlmid[b] = 1000 * (ri + 1) + 37 * b
        ids = np.sort(rng.permutation(int(nlmid[b]))[:m]).astype(np.int32)
        if it.get("order") == "desc":
            ids = ids[::-1]
        elif it.get("order") == "random":
            ids = rng.permutation(ids)
        if it.get("dup"):
            ids[7] = ids[3]
        px[b, :m], lmid[b, :m], n[b] = p, ids, m
        is3d[b, :m] = rng.uniform(size=m) < 0.6
        mk[b] = it.get("flag", 1)
        # what an unflagged item's slots hold is nobody's business: garbage behind and in them
        px[b, m:] = rng.uniform(-50, 500, (N_MAX - m, 2)); lmid[b, m:] = -7; is3d[b, m:] = 3
    Twc = np.array([np.concatenate([rng.normal(0, 1, 3), _unit(rng.normal(0, 1, 4))]) for _ in range(BATCH)])
    out = dict(px=px, lmid=lmid, is3d=is3d, n=n, make_kf=mk, nlmid=nlmid, nkfid=np.array([10 * ri + b for b in range(BATCH)], np.int32),
               time=np.array([10.0 + r["frame"] * 0.05 + 0.001 * ri] * BATCH), Twc=Twc)
    for a in out.values():
        a.setflags(write=False)
    return out


def _unit(q):
    return q / np.linalg.norm(q)
