"""Timings of the loop closer's keyframe preparation on the GPU (csrc/lckf.hip), each the median of --reps runs after a warm-up call:

    python tools/lckf_time.py [--reps N] [--out file.json] [--items 4096]

  host      ov2_lckf_prepare on one 752 x 480 keyframe with 300 exclusion points: staging upload of the image, the launches, the
            download and the synchronisation (host clock around the call)
  tracker   ov2_tracker_lckf_prepare on the same frame, which the tracker already holds on the device
  b11 / bN  ov2_lckf_prepare_batch_d on 11 and on --items resident frames (16 distinct frames repeated, 300 exclusion points and 512
            kept slots per item): the host clock around the call (wall) and the time between two events recorded on the context's
            stream around it (device), per call and per item
and two yardsticks from the same session: one read of the image at the HBM rate (752 * 480 B at 8 TB/s), and ov2_detect_grid_fast_d
(the front end's detector, cells of 35 pixels) on level 0 of the same frame's pyramid.  Prints one JSON line.  No assertion: nobody
has fixed a figure for this yet."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BPS = 8.0e12
W, H, N_EXCL, KEPT_CAP = 752, 480, 300, 512


def median_us(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e6


class Hip:
    """the few runtime calls the batch measurement needs (the runtime the library is linked against)"""

    def __init__(self):
        self.lib = C.CDLL("libamdhip64.so")
        self.lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.lib.hipFree.argtypes = [C.c_void_p]
        self.lib.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        self.lib.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        self.lib.hipEventSynchronize.argtypes = [C.c_void_p]
        self.lib.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.bufs = []

    def ok(self, rc):
        if rc != 0:
            raise RuntimeError("HIP error %d" % rc)

    def malloc(self, nbytes):
        p = C.c_void_p()
        self.ok(self.lib.hipMalloc(C.byref(p), max(int(nbytes), 1)))
        self.bufs.append(p)
        return p.value

    def put(self, dst, a):
        a = np.ascontiguousarray(a)
        self.ok(self.lib.hipMemcpy(C.c_void_p(dst), a.ctypes.data_as(C.c_void_p), a.nbytes, 1))

    def event(self):
        e = C.c_void_p()
        self.ok(self.lib.hipEventCreate(C.byref(e)))
        return e

    def free(self):
        for p in self.bufs:
            self.lib.hipFree(p)
        self.bufs = []


def batch(ctx, hip, LC, frames, excl, items, reps):
    """(wall us, device us) of ov2_lckf_prepare_batch_d on `items` resident frames"""
    nb = len(frames)
    d_img = hip.malloc(items * W * H)
    d_ex = hip.malloc(items * N_EXCL * 8)
    d_n = hip.malloc(items * 4)
    for b0 in range(0, items, nb):
        k = min(nb, items - b0)
        hip.put(d_img + b0 * W * H, frames[:k]); hip.put(d_ex + b0 * N_EXCL * 8, excl[:k])
    hip.put(d_n, np.full(items, N_EXCL, np.int32))
    d_kxy, d_kr, d_kv = hip.malloc(items * KEPT_CAP * 4), hip.malloc(items * KEPT_CAP), hip.malloc(items * KEPT_CAP)
    d_kd, d_cnt = hip.malloc(items * KEPT_CAP * 32), hip.malloc(items * 16)
    p = LC.lckf_params()
    e0, e1 = hip.event(), hip.event()
    stream = C.c_void_p(ctx.stream)
    dev = []

    def call():
        hip.ok(hip.lib.hipEventRecord(e0, stream))
        LC.lckf_prepare_batch_d(ctx, p, d_img, W, H, W, W * H, items, d_ex, N_EXCL, d_n, 0, 0, 0, d_kxy, d_kr, d_kv, d_kd, KEPT_CAP, d_cnt)
        hip.ok(hip.lib.hipEventRecord(e1, stream))
        hip.ok(hip.lib.hipEventSynchronize(e1))
        ms = C.c_float(0)
        hip.ok(hip.lib.hipEventElapsedTime(C.byref(ms), e0, e1))
        dev.append(ms.value * 1e3)
    wall = median_us(call, reps)
    hip.free()
    return wall, float(np.median(dev[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--items", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import ov2slam_amd
    from ov2slam_amd import loop_closer as LC
    from ov2slam_amd import synth
    ctx = ov2slam_amd.Context(0)
    tex = synth.base_texture(seed=2)
    frames = np.stack([synth.frame_pair(W, H, tex=tex, shift=(5.0 * k, -3.0 * k))[1] for k in range(16)])
    rng = np.random.default_rng(0)
    excl = np.stack([np.stack([rng.uniform(0, W, N_EXCL), rng.uniform(0, H, N_EXCL)], axis=1) for _ in range(16)]).astype(np.float32)
    img, e = frames[0], excl[0]
    p = LC.lckf_params()
    one = LC.lckf_prepare(ctx, p, img, e)
    res = dict(w=W, h=H, n_excl=N_EXCL, n_all=one["n_all"], n_kept=one["n_kept"], n_desc=one["n_desc"],
               image_read_us_at_8TBps=W * H / HBM_BPS * 1e6)
    res["host_us"] = median_us(lambda: LC.lckf_prepare(ctx, p, img, e, kept_cap=KEPT_CAP), a.reps)
    vt = ov2slam_amd.VisualFrontEndTracker(ctx, W, H, use_clahe=True)
    vt.trackFrame(img, np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), None)
    res["tracker_us"] = median_us(lambda: LC.lckf_prepare_tracker(vt, p, e, kept_cap=KEPT_CAP), a.reps)
    fx = ov2slam_amd.FeatureExtractor(ctx)
    res["detect_grid_fast_d_us"] = median_us(lambda: fx.detectGridFASTPyr(vt.cur_pyr, 35, np.zeros((0, 2), np.float32)), a.reps)
    vt.close()
    hip = Hip()
    for items in (11, a.items):
        wall, dev = batch(ctx, hip, LC, frames, excl, items, a.reps if items <= 64 else max(3, a.reps // 6))
        k = "b%d" % items
        res.update({k + "_wall_us": wall, k + "_device_us": dev, k + "_wall_us_per_item": wall / items, k + "_device_us_per_item": dev / items,
                    k + "_device_over_image_read": dev / items / res["image_read_us_at_8TBps"]})
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
