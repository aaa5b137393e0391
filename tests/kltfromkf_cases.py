"""Scenes for VisualFrontEnd::kltTrackingFromKF (plain numpy + the CPU oracle), built to populate every branch of its data path: what
tests/test_kltfromkf_cases.py checks on the oracle alone and tests/test_gpu_kltfromkf.py runs through the lock-step tracker.

A case is one step of a tracker of BATCH items of which N_ACTIVE take part.  Per item: a keyframe image and a current image cut
from one texture a few pixels and a fraction of a degree apart, the keyframe's table (ids ascending, px), the ids taken out of the
keyframe since (REMOVE_OBS), and the frame: per slot an id, the px the frame carries (the track of the frame before: a pixel or two
off the truth), whether the map has a 3-D point for it and where that point projects.  Projections are good (half a pixel off the
truth), far (12 to 20 px off, 45 to 70 px on the item where the 33 % rule is to fire: the one-level pass loses most of them, the
retry from the frame's px finds them) or lie on a patch of the
current image that shows something else (lost by both passes).  3-D points are given in the camera frame of an identity pose, so
the projection the device computes is the designed one up to rounding.  Frame size and slots: those of tests/test_gpu_resident.py."""
import functools

import numpy as np

from ov2slam_amd import synth

W, H, N_MAX, BATCH, N_ACTIVE = 376, 240, 160, 5, 4
K = (229.327, 228.648, 183.6075, 124.1875)                         # EuRoC halved, no distortion
SHIFT, THETA = (6.5, -3.0), 0.01                                   # keyframe -> current frame
PATCH = (230, 300, 60, 120)                                        # x0, x1, y0, y1 of the current image replaced by another texture

# per item: slots in the keyframe, slots the table never held, slots whose id was removed from the keyframe, share of 3-D slots,
# share of the 3-D slots whose projection is far off, points on the replaced patch
ITEMS = {
    "mixed":    dict(n_in=90, n_new=7, n_removed=5, p3d=0.7, pfar=0.25, n_patch=8),
    "rule":     dict(n_in=64, n_new=0, n_removed=0, p3d=0.7, pfar=0.97, n_patch=0, far=(45, 70)),
    "outside":  dict(n_in=0, n_new=30, n_removed=7, p3d=0.7, pfar=0.0, n_patch=0),
    "full":     dict(n_in=N_MAX, n_new=0, n_removed=0, p3d=0.6, pfar=0.1, n_patch=4),
    "empty":    dict(n_in=0, n_new=0, n_removed=0, p3d=0.0, pfar=0.0, n_patch=0),
    "one":      dict(n_in=1, n_new=0, n_removed=0, p3d=1.0, pfar=0.0, n_patch=0),
    "wave65":   dict(n_in=63, n_new=2, n_removed=0, p3d=0.5, pfar=0.3, n_patch=0),
}
# name -> the four active items, klt_use_prior
SPECS = {
    "main":    dict(items=("mixed", "rule", "outside", "full"), use_prior=True),
    "edges":   dict(items=("empty", "one", "wave65", "mixed"), use_prior=True),
    "noprior": dict(items=("mixed", "rule", "outside", "full"), use_prior=False),
}
NAMES = tuple(SPECS)


def flow(pts, frac=1.0):
    """where the scene points seen at pts in the keyframe lie after the share `frac` of the motion to the current frame"""
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    p = np.asarray(pts, np.float64).reshape(-1, 2)
    dx, dy = p[:, 0] - cx - frac * SHIFT[0], p[:, 1] - cy - frac * SHIFT[1]
    c, s = np.cos(-frac * THETA), np.sin(-frac * THETA)
    return np.stack([c * dx - s * dy + cx, s * dx + c * dy + cy], 1)


@functools.lru_cache(maxsize=None)
def images(seed):
    tex = synth.base_texture(max(W, H) + 500, seed)
    kf = synth.warp(tex, W, H, 120.0, 110.0, 0.0)
    cur = synth.warp(tex, W, H, 120.0 + SHIFT[0], 110.0 + SHIFT[1], THETA).copy()
    x0, x1, y0, y1 = PATCH
    cur[y0:y1, x0:x1] = synth.warp(synth.base_texture(max(W, H) + 500, seed + 1000), W, H, 40.0, 50.0, 0.3)[y0:y1, x0:x1]
    return kf, cur


def unproject(px, depth):
    """camera-frame points that project onto px under K (no distortion): with the identity pose, the world points"""
    px = np.asarray(px, np.float64).reshape(-1, 2)
    z = np.asarray(depth, np.float64).reshape(-1)
    return np.stack([(px[:, 0] - K[2]) / K[0] * z, (px[:, 1] - K[3]) / K[1] * z, z], 1)


@functools.lru_cache(maxsize=None)
def item(kind, seed):
    s = ITEMS[kind]
    rng = np.random.default_rng(seed)
    kf_img, cur_img = images(seed)
    n_in, n_new, n_rm = s["n_in"], s["n_new"], s["n_removed"]
    n_tab = min(n_in + n_rm + 5, N_MAX)                                    # the table holds ids the frame has lost long ago, too
    ids = np.sort(rng.choice(100000, n_tab + n_new, replace=False)).astype(np.int32)
    new_ids = rng.choice(ids, n_new, replace=False) if n_new else np.zeros(0, np.int32)
    tab_lmid = np.array([v for v in ids if v not in set(new_ids.tolist())], np.int32)
    tab_px = np.stack([rng.uniform(24, W - 24, n_tab), rng.uniform(24, H - 24, n_tab)], 1).astype(np.float32)
    x0, x1, y0, y1 = PATCH
    for k in range(min(s["n_patch"], n_in)):                               # their truth in the current frame lies on the patch
        tab_px[k] = (rng.uniform(x0 + 14, x1 - 14) + SHIFT[0], rng.uniform(y0 + 14, y1 - 14) + SHIFT[1])
    order = rng.permutation(n_tab)
    in_slots, rm_slots = np.sort(order[:n_in]), order[n_in:n_in + n_rm]
    if s["n_patch"]:
        in_slots = np.sort(np.unique(np.concatenate([np.arange(min(s["n_patch"], n_in)), in_slots]))[:n_in]) if n_in else in_slots
    rm_slots = np.array([v for v in order if v not in set(in_slots.tolist())][:n_rm], np.int64)
    members = np.ones(n_tab, bool)
    members[rm_slots] = False
    # the frame: the slots in a random order
    f_tab = np.concatenate([in_slots, rm_slots]).astype(np.int64)
    lmid = np.concatenate([tab_lmid[f_tab], new_ids]).astype(np.int32)
    src = np.concatenate([tab_px[f_tab], np.stack([rng.uniform(24, W - 24, n_new), rng.uniform(24, H - 24, n_new)], 1).reshape(-1, 2)])
    n = len(lmid)
    perm = rng.permutation(n)
    lmid, src = lmid[perm], src[perm]
    truth = flow(src)
    px = (flow(src, 0.7) + rng.normal(0, 0.4, (n, 2))).astype(np.float32)
    is3d = rng.random(n) < s["p3d"]
    far = is3d & (rng.random(n) < s["pfar"])
    proj = truth + rng.normal(0, 0.5, (n, 2))
    proj[far] += (rng.uniform(*s.get("far", (12, 20)), (n, 1)) * np.array([[0.8, -0.6]]))[far]
    proj = proj.astype(np.float32)
    in_img = (proj[:, 0] >= 0) & (proj[:, 1] >= 0) & (proj[:, 0] < W) & (proj[:, 1] < H)
    wpt = unproject(proj, rng.uniform(2, 10, n))
    return dict(kind=kind, kf_img=kf_img, cur_img=cur_img, tab_lmid=tab_lmid, tab_px=tab_px, members=members, n=n, lmid=lmid, px=px,
                is3d=is3d.astype(np.uint8), wpt=wpt, proj=proj, has_prior=(is3d & in_img).astype(np.uint8), truth=truth)


def case(name):
    s = SPECS[name]
    return dict(name=name, use_prior=s["use_prior"], items=[item(kind, 500 + 10 * k) for k, kind in enumerate(s["items"])])


def pyramids(O, it, clahe=False):
    a, b = it["kf_img"], it["cur_img"]
    if clahe:
        a, b = O.clahe(a, 3.0, W // 50, H // 50), O.clahe(b, 3.0, W // 50, H // 50)
    return O.Pyramid(a, 9, 3), O.Pyramid(b, 9, 3)


def reference(O, it, use_prior, clahe=False, proj=None, has_prior=None, **kw):
    """kltfromkf_ref on the item: the keyframe is the table's entries that are still members"""
    from tests import kltfromkf_ref as R
    kp, cp = pyramids(O, it, clahe)
    m = it["members"]
    return R.klt_tracking_from_kf(kp, cp, it["px"], it["lmid"], it["tab_lmid"][m], it["tab_px"][m], it["proj"] if proj is None else proj,
                                  it["has_prior"] if has_prior is None else has_prior, klt_use_prior=use_prior, **kw)
