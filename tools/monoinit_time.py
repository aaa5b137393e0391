"""Time of the mono initialisation test (trackMono's un-initialised branch with checkReadyForInit) for the flagged items of a lock-step
batch as one call (ov2_btracker_mono_init) against the route of separate calls it replaces, and of the stand-alone single call:
S sequences, 308 slots per item against a keyframe of 308 keypoints (tests/epifilter_ref.geo_scene: two views of a point cloud, 60
planted mismatches, 20 ids the keyframe does not hold), 100 iterations over 200 rows:

    python tools/monoinit_time.py [S] [calls] [--flag all|fifth] [--out FILE]

The method of tools/temporalkf_time.py: one process, the forms alternate call by call, every call is timed on its own and ends in its
own host synchronisation; the median and the quartiles of all timed calls are reported.  In front of every timed call of any form,
outside the timed region, the frames and poses of the flagged items are installed again (setFrame, setPose), so that every call
does the same work: every flagged item searches, is READY and loses its outliers.  --flag fifth: one item in five is flagged.
  fused        ov2_btracker_mono_init
  route_calls  the route's C calls alone, on arguments that lie ready: ov2_parallax_batch, ov2_epipolar_ransac_batch,
               ov2_btracker_update_frame_batch, and ov2_btracker_set_pose + ov2_btracker_reset_motion per flagged item.  A lower
               bound of any route.
  route_host   the route with its host work (tests/monoinit_ref.route): getFrame and ov2_compute_keypoints per flagged item, the
               join and the K rotbv parallax in numpy, ov2_epipolar_draw_samples, composing the REMOVE ops, and the calls above.
  single       ov2_mono_init on one item (no tracker)
Prints one JSON line (and appends it to --out; profiles/monoinit_time.json holds the lines of the four cases).  The time of the
sample-table draw that this call shares with k_epif_gather, against the revision before the draw moved, is tools/epif_draw_ab.sh."""
import json
import os
import sys
import time

import numpy as np

argv = list(sys.argv[1:])
TREE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT = {"--flag": "all", "--out": None}
for flag in list(OPT):
    if flag in argv:
        i = argv.index(flag)
        OPT[flag] = argv[i + 1]
        del argv[i:i + 2]
sys.path.insert(0, TREE)

import ov2slam_amd                                                 # noqa: E402
from ov2slam_amd import _lib as L                                  # noqa: E402
from ov2slam_amd import keyframe, pose                             # noqa: E402
from tests import epifilter_ref as EF                              # noqa: E402
from tests import kfreq_ref as KF                                  # noqa: E402
from tests import monoinit_ref as R                                # noqa: E402

S = int(argv[0]) if len(argv) > 0 else 4096
CALLS = int(argv[1]) if len(argv) > 1 else 6
FLAG, OUT = OPT["--flag"], OPT["--out"]
W, H, N, ROWS = 752, 480, 308, 200


def stats(ms):
    q = np.percentile(np.array(ms), [25, 50, 75])
    return dict(median_ms=round(float(q[1]), 4), q1_ms=round(float(q[0]), 4), q3_ms=round(float(q[2]), 4), n=len(ms))


def main():
    ctx = ov2slam_amd.Context(0)
    Kc = KF.EUROC_K
    cal = ov2slam_amd.CameraCalibration(ctx, "pinhole", *Kc, D=None)
    t = ov2slam_amd.LockstepTracker(ctx, S, W, H, use_clahe=False, nbmaxkps=N)
    t.setCalibration(cal)
    P = R.make_P(n_rows=ROWS, max_iterations=100, min_2d_kps=50, finit_parallax=10.0)
    scenes = []
    for c in range(8):                                              # 8 contents, spread over the items
        cur, kf = EF.geo_scene(900 + c, N, outliers=60, unknown=20)
        it = R.flatten(cur, kf)
        scenes.append(dict(item=it, px=it["cur_unpx"].copy(), wpt=np.zeros((N, 3)),
                           kf=dict(lmid=it["kf_lmid"], unpx=it["kf_unpx"], bv=it["kf_bv"], Twc=np.array(kf["Twc"], np.float64))))
    do = np.ones(S, np.uint8) if FLAG == "all" else (np.arange(S) % 5 == 0).astype(np.uint8)
    flagged = [b for b in range(S) if do[b]]
    seeds = (np.arange(S, dtype=np.uint64) * np.uint64(2) + np.uint64(1))
    kfs = []
    for b in range(S):
        sc = scenes[b % 8]
        t.setKeyframe(b, sc["kf"]["lmid"], sc["kf"]["unpx"], sc["kf"]["bv"], sc["kf"]["Twc"])
        t.setKeyframeInfo(b, 100 + b, 10.0, 0)
        kfs.append(sc["kf"])

    def restore():
        for b in flagged:
            sc = scenes[b % 8]
            t.setFrame(b, sc["px"], sc["item"]["cur_lmid"], sc["item"]["cur_is3d"], sc["wpt"])
            t.setPose(b, sc["item"]["cur_Twc"])
        ctx.sync()

    # the arguments of route_calls, ready: the items of the parallax, the problems of the search, the REMOVE ops, the poses
    restore()
    removed = np.zeros((S, N), np.uint8)
    recs, removed = R.route(ctx, t, cal, S, do, seeds, P, kfs, removed)
    assert all(recs[b]["action"] == R.READY for b in flagged), sorted({recs[b]["action"] for b in flagged})
    items = [dict(scenes[b % 8]["item"]) for b in flagged]
    probs = []
    for b in flagged:
        it = scenes[b % 8]["item"]
        j = np.searchsorted(it["kf_lmid"], it["cur_lmid"])
        hit = (j < len(it["kf_lmid"])) & (it["kf_lmid"][np.minimum(j, len(it["kf_lmid"]) - 1)] == it["cur_lmid"])
        pc = np.nonzero(hit)[0]
        probs.append(dict(bv1=it["kf_bv"][j[pc]], bv2=it["cur_bv"][pc], samples=pose.epipolar_draw_samples(int(seeds[b]), len(pc), ROWS)))
    ops = [[(int(scenes[b % 8]["item"]["cur_lmid"][i]), L.OV2_RES_REMOVE, None) for i in np.nonzero(removed[b])[0]] if do[b] else [] for b in range(S)]
    epp = pose.epipolar_params(P["max_iterations"], P["threshold"], P["probability"])

    def fused():
        t.monoInit(S, do, seeds, P)

    def route_calls():
        keyframe.parallax_batch(ctx, P["fkf"], items, unrot=0, filter=keyframe.ALL, stat=keyframe.MEDIAN)
        pose.epipolar_ransac_batch(ctx, epp, probs)
        t.updateFrame(S, ops)
        for b in flagged:
            t.setPose(b, recs[b]["Twc_init"])
            t.resetMotion(b)

    def route_host():
        R.route(ctx, t, cal, S, do, seeds, P, kfs, removed)

    forms = dict(fused=fused, route_calls=route_calls, route_host=route_host)
    ms = {k: [] for k in forms}
    for k in range(CALLS + 1):                                      # the first round warms up
        for name, fn in forms.items():
            restore()
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if k:
                ms[name].append(dt)
    single = []
    for k in range(4 * CALLS + 1):
        t0 = time.perf_counter()
        r = keyframe.mono_init(ctx, P, scenes[0]["item"])
        dt = (time.perf_counter() - t0) * 1e3
        if k:
            single.append(dt)
    assert r["action"] == R.READY
    restore()
    fused()
    slot_bytes = int(t.lastSlotBytes())
    out = dict(tool="monoinit_time", sequences=S, flag=FLAG, flagged=len(flagged), slots=N, rows=ROWS, max_iterations=100,
               n_removed=int(recs[flagged[0]]["n_removed"]), m=int(recs[flagged[0]]["m"]), slot_bytes_fused=slot_bytes,
               forms={k: stats(v) for k, v in ms.items()}, single=stats(single))
    t.close()
    line = json.dumps(out)
    print(line)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
