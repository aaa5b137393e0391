"""The lock-step pose step (ov2_btracker_track_frame_pose, scope row f16) as a specification in numpy and existing wrappers:
   pose_set       which slots of an item enter computePose, in which order
   draw_samples   ov2_p3p_draw_samples restated (splitmix64 over a running counter, % n, duplicates within a row rejected), and the
                  same table by the scheme the device uses (draw_samples_by_lanes)
   route          the separate calls the fused step replaces: trackFrameMap -> pose_set on the host -> ov2_p3p_draw_samples ->
                  pose.compute_pose_batch -> the removal bytes scattered back to slot space
The GPU test holds the fused step to route() byte for byte."""
import numpy as np

from ov2slam_amd import pose

_M64 = (1 << 64) - 1


def pose_set(status, is3d, n):
    """the slots i < n with (status[i] & 3) == 1 and is3d[i], ascending"""
    s, d = np.asarray(status)[:n], np.asarray(is3d)[:n]
    return np.nonzero(((s & 3) == 1) & (d != 0))[0].astype(np.int32)


def splitmix64(seed, j):
    z = (seed + (j + 1) * 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def draw_samples(seed, n, rows):
    """(rows, 4) int32: the integers of ov2_p3p_draw_samples(seed, n, rows)"""
    assert n >= 4 and rows >= 0
    seed = int(seed) & _M64
    out = np.zeros((rows, 4), np.int32)
    j = 0
    for r in range(rows):
        row = []
        while len(row) < 4:
            v = splitmix64(seed, j) % n
            j += 1
            if v not in row:
                row.append(v)
        out[r] = row
    return out


def draw_samples_by_lanes(seed, n, rows, lanes=64, walk=4096):
    """the same table by the scheme of k_pose_pack: `lanes` rows at a time, row l from counter j0 + 4 l as if no earlier row rejected a
    value; the rows up to and including the first that consumed more than four values are right, the rest is drawn again"""
    seed = int(seed) & _M64
    out, j0, done = np.zeros((rows, 4), np.int32), 0, 0
    for _ in range(rows + 8):
        if done >= rows:
            break
        rws, cnts = [], []
        for l in range(lanes):
            row, cnt = [], 0
            while len(row) < 4 and cnt < walk:
                v = splitmix64(seed, j0 + 4 * l + cnt) % n
                cnt += 1
                if v not in row:
                    row.append(v)
            rws.append(row); cnts.append(cnt)
        first = next((l for l in range(lanes) if cnts[l] != 4), lanes)
        take = first + (1 if len(rws[first]) == 4 else 0) if first < lanes else lanes
        take = min(take, rows - done)
        if take <= 0:
            break
        out[done:done + take] = rws[:take]
        j0 += 4 * first + cnts[first] if take == first + 1 else 4 * take
        done += take
    return out[:done]


def nothing_ran(Twc, p3p_req, n):
    """what the step returns for an item on a tracker's first frame and on a step where nothing is tracked"""
    z = dict(ran=False, iterations=0, num_successful_steps=0, termination=0, initial_cost=0.0, final_cost=0.0)
    return dict(Twc=np.array(Twc, np.float64), action=pose.TOO_FEW, p3p_req_out=bool(p3p_req), removed=np.zeros(n, np.uint8),
                n_removed_p3p=0, n_outliers_pnp=0, ran_p3p=False,
                p3p=dict(status=0, best_row=0, iterations=0, rows_consumed=0, score=0.0), passes=[dict(z), dict(z)])


def route(ctx, trk, imgs, kps, wpt, is3d, Tcw, n, params, Twc, p3p_req, seed, scale=None, dop3p=False, n_rows=0, klt_use_prior=True):
    """-> (out, status, p3p flags of the rule, poses, inputs): poses[b] as pose.compute_pose returns it with removed (n[b],) in slot
    space; inputs[b] = (m, slots, samples) as they were fed"""
    out, st, rule = trk.trackFrameMap(imgs, kps, wpt, is3d, Tcw, n, klt_use_prior=klt_use_prior)
    na = len(imgs)
    wpt = np.asarray(wpt, np.float64).reshape(trk.batch, trk.n_max, 3)
    is3d = np.asarray(is3d, np.uint8).reshape(trk.batch, trk.n_max)
    problems, inputs = [], []
    for b in range(na):
        nb = int(n[b])
        slots = pose_set(st[b], is3d[b], nb)
        m = len(slots)
        unpx, bv = trk.lastKeypoints(b, nb) if nb else (np.zeros((0, 2), np.float32), np.zeros((0, 3)))
        req = bool(p3p_req[b]) or bool(rule[b])
        do_p3p = req or bool(dop3p)
        tab = pose.draw_samples(int(seed[b]), m, n_rows) if do_p3p and m >= 4 else np.zeros((0, 4), np.int32)
        sc = np.zeros(m, np.int32) if scale is None else np.asarray(scale, np.int32).reshape(trk.batch, trk.n_max)[b, slots]
        problems.append(dict(unpx=unpx[slots].astype(np.float64), wpt=wpt[b, slots], scale=sc, Twc=np.asarray(Twc, np.float64).reshape(-1, 7)[b],
                             bv=bv[slots], do_p3p=do_p3p, p3p_req=req, samples=tab))
        inputs.append((m, slots, tab))
    poses = pose.compute_pose_batch(ctx, params, problems)
    for b in range(na):
        nb = int(n[b])
        rm = np.zeros(nb, np.uint8)
        rm[inputs[b][1]] = poses[b]["removed"]
        poses[b]["removed"] = rm
    return out, st, rule, poses, inputs


def pose_bytes(p):
    """every field of a pose result, as bytes, field by field (so that a failing comparison names the field)"""
    d = dict(Twc=np.asarray(p["Twc"], np.float64).tobytes(), action=int(p["action"]), p3p_req_out=bool(p["p3p_req_out"]),
             n_removed_p3p=int(p["n_removed_p3p"]), n_outliers_pnp=int(p["n_outliers_pnp"]), ran_p3p=bool(p["ran_p3p"]),
             removed=np.asarray(p["removed"], np.uint8).tobytes())
    for k in ("status", "best_row", "iterations", "rows_consumed"):
        d["p3p_" + k] = int(p["p3p"][k])
    d["p3p_score"] = np.float64(p["p3p"]["score"]).tobytes()
    for q in range(2):
        for k in ("ran", "iterations", "num_successful_steps", "termination"):
            d["pass%d_%s" % (q, k)] = int(p["passes"][q][k])
        for k in ("initial_cost", "final_cost"):
            d["pass%d_%s" % (q, k)] = np.float64(p["passes"][q][k]).tobytes()
    return d
