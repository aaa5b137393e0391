"""GPU parity of the device rectification (ov2_rectmap_*, ov2_rectify_h / _d, ov2_*_set_rectification, ov2_pyr_build_rect_h;
csrc/rectify.hip: k_remap) against tests/remap_ref.py -- the restatement of cv::remap (CV_8UC1, INTER_LINEAR, BORDER_CONSTANT 0)
behind CameraCalibration::rectifyImage (the reference's src/camera_calibration.cpp:233-241).  Bit for bit everywhere: a tracker
that rectifies on the device and is fed RAW frames must return exactly what a tracker without rectification returns on
remap_ref(raw)."""
import ctypes as C
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import ov2slam_amd
from ov2slam_amd import synth, stereo
from ov2slam_amd import _lib as L

from tests import remap_ref as R
from tests.test_gpu_tracker import _sequence, _points, _bits, CLIP

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

IMAGES = ["noise83x37", "noise257x300", "noise121x99", "synth752x480", "synth1241x376"]
MAPS = ["identity", "shift", "euroc", "wild", "edge"]
SRC_CANARY, DST_CANARY = 0xA5, 0x5A


@functools.lru_cache(maxsize=None)
def _image(name):
    kind, wh = name[:5], name[5:]
    w, h = (int(v) for v in wh.split("x"))
    if kind == "noise":
        return np.random.default_rng(w * 7 + h).integers(0, 256, (h, w), dtype=np.uint8)
    return np.ascontiguousarray(synth.frame_pair(w, h, seed=w + h)[0])


@functools.lru_cache(maxsize=None)
def _maps(name, w, h):
    """-> {"f32": (x, y), "fixed": (ixy, ab)}"""
    if name == "identity":
        m = R.identity_maps(w, h)
    elif name == "shift":
        m = R.shift_maps(w, h, 3, -2)
    elif name == "euroc":
        m = R.euroc_like_maps(w, h)
    elif name == "wild":
        m = R.wild_maps(w, h)
    else:
        m = R.edge_maps(w, h)
    return R.both_forms(*m)


@functools.lru_cache(maxsize=None)
def _ref(img_name, map_name):
    img = _image(img_name)
    h, w = img.shape
    out = R.remap(img, "f32", *_maps(map_name, w, h)["f32"])
    out.setflags(write=False)
    return out


def _strided(img, stride, fill):
    buf = np.full((img.shape[0], stride), fill, np.uint8)
    buf[:, :img.shape[1]] = img
    return buf


def _up16(v):
    return (v + 15) & ~15


@pytest.mark.parametrize("map_name", MAPS)
@pytest.mark.parametrize("img_name", IMAGES)
def test_rectify_h_matches_reference(gpu_ctx, img_name, map_name):
    img = _image(img_name)
    h, w = img.shape
    ref = _ref(img_name, map_name)
    if map_name == "identity":
        assert np.array_equal(ref, img)
    if map_name in ("wild", "edge"):
        mx, my = _maps(map_name, w, h)["f32"]
        assert mx.min() < -1 and my.min() < -1 and mx.max() >= w and my.max() >= h     # the map leaves the image on every side
        assert (ref == 0).any() and (ref != 0).any()
    # the fixed form of a map is what the f32 form normalises to: one reference serves both
    assert np.array_equal(R.remap(img, "fixed", *_maps(map_name, w, h)["fixed"]), ref)
    src = _strided(img, w + 13, SRC_CANARY)
    # a destination pitch equal to the library's own staging pitch (width rounded up to 16) where that leaves padding, w + 7 otherwise
    dstride = _up16(w) if w % 16 else w + 7
    for form in ("f32", "fixed"):
        rm = ov2slam_amd.RectifyMap(gpu_ctx, form, *_maps(map_name, w, h)[form])
        dst = np.full((h, dstride), DST_CANARY, np.uint8)
        rm.rectify(src[:, :w], out=dst[:, :w])
        assert np.array_equal(dst[:, :w], ref), "%s %s %s" % (img_name, map_name, form)
        assert (dst[:, w:] == DST_CANARY).all() and (src[:, w:] == SRC_CANARY).all() and np.array_equal(src[:, :w], img)
        rm.close()


@pytest.mark.parametrize("w,h", [(2, 2), (7, 3), (8, 5), (9, 2), (12, 17)])
def test_rectify_h_narrow_images(gpu_ctx, w, h):
    """Below 8 columns the kernel gathers every pair of source pixels on its own; from 8 on a lane whose footprint is compact reads
    whole 8-byte row segments, which at these widths start at the clamped column w - 8"""
    img = np.random.default_rng(w * 31 + h).integers(0, 256, (h, w), dtype=np.uint8)
    u, v = R.identity_maps(w, h)
    for mx, my in ((u, v), (u + np.float32(0.75), v - np.float32(0.25)), (u * np.float32(0.5) - np.float32(1.25), v * np.float32(0.5) + np.float32(h / 2.0)),
                   R.shift_maps(w, h, 1, 1)):
        f = R.both_forms(mx, my)
        ref = R.remap(img, "f32", *f["f32"])
        rm = ov2slam_amd.RectifyMap(gpu_ctx, "f32", *f["f32"])
        dst = np.full((h, w + 3), DST_CANARY, np.uint8)
        rm.rectify(img, out=dst[:, :w])
        assert np.array_equal(dst[:, :w], ref) and (dst[:, w:] == DST_CANARY).all()
        rm.close()


@pytest.mark.parametrize("img_name,map_name", [("noise83x37", "wild"), ("noise121x99", "edge"), ("synth752x480", "euroc")])
def test_rectify_h_in_place(gpu_ctx, img_name, map_name):
    img = _image(img_name)
    h, w = img.shape
    rm = ov2slam_amd.RectifyMap(gpu_ctx, "fixed", *_maps(map_name, w, h)["fixed"])
    buf = _strided(img, w + 5, SRC_CANARY)
    out = rm.rectify(buf[:, :w], out=buf[:, :w])                         # dst_h == src_h: the reference rectifies in place
    assert out.ctypes.data == buf.ctypes.data
    assert np.array_equal(buf[:, :w], _ref(img_name, map_name)) and (buf[:, w:] == SRC_CANARY).all()
    rm.close()


class _Hip:
    """hipMalloc / hipMemcpy of the runtime the library is linked against (device buffers for ov2_rectify_d)"""

    def __init__(self):
        self.lib = C.CDLL("libamdhip64.so")
        self.lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.lib.hipFree.argtypes = [C.c_void_p]
        self.bufs = []

    def upload(self, a):
        p = C.c_void_p()
        assert self.lib.hipMalloc(C.byref(p), a.nbytes) == 0
        self.bufs.append(p)
        assert self.lib.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0
        return p.value

    def download(self, ptr, a):
        assert self.lib.hipMemcpy(a.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), a.nbytes, 2) == 0
        return a

    def free(self):
        for p in self.bufs:
            self.lib.hipFree(p)
        self.bufs = []


def _items(n, w, h, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(n)]


def _pack_items(imgs, pitch, item_stride, fill, n_slots):
    h, w = imgs[0].shape
    buf = np.full(n_slots * item_stride, fill, np.uint8)
    for b, im in enumerate(imgs):
        buf[b * item_stride:b * item_stride + h * pitch].reshape(h, pitch)[:, :w] = im
    return buf


# (w, h, slots, n_items, src pitch, src item slack, dst pitch, dst item slack): whole-dword stores (dst pitch and item stride multiples
# of 4), byte stores (an odd dst pitch), and more items than one work-group serves (several item groups, the last one short)
@pytest.mark.parametrize("w,h,slots,n_items,sp,ss,dp,ds", [(376, 240, 5, 3, 384, 128, 380, 64), (376, 240, 5, 3, 379, 3, 377, 5),
                                                          (83, 37, 39, 37, 96, 32, 84, 12)])
def test_rectify_d_items_and_strides(gpu_ctx, w, h, slots, n_items, sp, ss, dp, ds):
    imgs = _items(slots, w, h, w + n_items)
    maps = _maps("wild" if w == 83 else "euroc", w, h)
    s_item, d_item = sp * h + ss, dp * h + ds                             # item strides != h * pitch
    src = _pack_items(imgs, sp, s_item, SRC_CANARY, slots)
    dst0 = np.full(slots * d_item, DST_CANARY, np.uint8)
    hip = _Hip()
    rm = ov2slam_amd.RectifyMap(gpu_ctx, "f32", *maps["f32"])
    try:
        d_src, d_dst = hip.upload(src), hip.upload(dst0)
        with pytest.raises(ov2slam_amd.Ov2Error):
            rm.rectify_device(d_src, sp, s_item, n_items, d_src, dp, d_item)          # src == dst
        with pytest.raises(ov2slam_amd.Ov2Error):
            rm.rectify_device(d_src, w - 1, s_item, n_items, d_dst, dp, d_item)       # stride below the width
        rm.rectify_device(d_src, sp, s_item, n_items, d_dst, dp, d_item)
        gpu_ctx.sync()
        got = hip.download(d_dst, np.empty_like(dst0))
    finally:
        rm.close()
        hip.free()
    exp = dst0.copy()
    for b in range(n_items):
        exp[b * d_item:b * d_item + h * dp].reshape(h, dp)[:, :w] = R.remap(imgs[b], "f32", *maps["f32"])
    # items [n_items, slots) of the destination, every row's padding and the slack between items keep their canary
    assert np.array_equal(got, exp)


def _tracker(ctx, w, h, use_graph, cal, rm=None, n_max=640, use_clahe=True):
    t = ov2slam_amd.VisualFrontEndTracker(ctx, w, h, use_clahe=use_clahe, fclahe_val=CLIP, nbmaxkps=n_max, use_graph=use_graph)
    t.setCalibration(cal)
    if rm is not None:
        t.setRectification(rm)
    return t


def _same_frame(A, B, ra, rb, n, label):
    """n: keypoints of the call (last_keypoints); BRIEF is taken on a fixed grid of points"""
    kps = synth.grid_keypoints(A.w, A.h, 35, np.random.default_rng(11))
    (ao, ast, ap), (bo, bst, bp) = ra, rb
    assert np.array_equal(_bits(ao), _bits(bo)) and np.array_equal(ast, bst) and ap == bp, label + ": positions / status"
    for lvl in (0, 2):
        assert np.array_equal(A.cur_pyr.download(lvl)[0], B.cur_pyr.download(lvl)[0]), label + ": pyramid level %d" % lvl
    (ad, av), (bd, bv) = A.describeBRIEF(kps), B.describeBRIEF(kps)
    assert np.array_equal(ad, bd) and np.array_equal(av, bv) and av.any(), label + ": describeBRIEF"
    if n:
        (au, ab_), (bu, bb) = A.lastKeypoints(n), B.lastKeypoints(n)
        assert np.array_equal(_bits(au), _bits(bu)) and np.array_equal(ab_.view(np.uint64), bb.view(np.uint64)), label + ": last_keypoints"


EMPTY = np.zeros((0, 2), np.float32)
K_EUROC = (458.654 / 2, 457.296 / 2, 367.215 / 2, 248.375 / 2)


@pytest.mark.parametrize("use_graph", [False, True])
def test_single_tracker_rectifies_in_its_enqueue(gpu_ctx, use_graph):
    """Tracker A (rectification set) on raw frames == tracker B (none) on remap_ref(raw), 4 frames"""
    w, h, nframes = 376, 240, 4
    raw, flow = _sequence(w, h, nframes, seed=21)
    maps = _maps("euroc", w, h)
    rect = [R.remap(f, "f32", *maps["f32"]) for f in raw]
    assert not np.array_equal(rect[0], raw[0])
    cal = ov2slam_amd.CameraCalibration(gpu_ctx, "pinhole", *K_EUROC)
    rm = ov2slam_amd.RectifyMap(gpu_ctx, "fixed", *maps["fixed"])
    other = ov2slam_amd.RectifyMap(gpu_ctx, "f32", *_maps("identity", w + 1, h)["f32"])
    A, B = _tracker(gpu_ctx, w, h, use_graph, cal, rm), _tracker(gpu_ctx, w, h, use_graph, cal)
    with pytest.raises(ov2slam_amd.Ov2Error) as e:
        B.setRectification(other)                                        # a map of another size
    assert e.value.code == L.OV2_EINVAL
    assert A.uses_graph == B.uses_graph
    rng = np.random.default_rng(3)
    _same_frame(A, B, A.trackFrame(_strided(raw[0], w + 9, SRC_CANARY), EMPTY, EMPTY, None), B.trackFrame(rect[0], EMPTY, EMPTY, None), 0, "frame 0")
    for f in range(1, nframes):
        k, p, hp = _points(w, h, flow, f - 1, rng, 1.0, bad_frac=0.2)
        ra, rb = A.trackFrame(raw[f], k, p, hp), B.trackFrame(rect[f], k, p, hp)
        assert (ra[1] & 1).mean() > 0.5
        _same_frame(A, B, ra, rb, len(k), "frame %d" % f)
    for t in (A, B):
        t.close()
    rm.close(); other.close()


@pytest.mark.parametrize("use_graph", [False, True])
def test_single_tracker_set_and_unset_between_frames(gpu_ctx, use_graph):
    """The map is set after frame 2 and unset (NULL) after frame 3: each frame is processed as its setting says"""
    w, h, nframes = 376, 240, 4
    raw, flow = _sequence(w, h, nframes, seed=22)
    maps = _maps("euroc", w, h)
    fed_b = [raw[0], raw[1], R.remap(raw[2], "f32", *maps["f32"]), raw[3]]
    cal = ov2slam_amd.CameraCalibration(gpu_ctx, "pinhole", *K_EUROC)
    rm = ov2slam_amd.RectifyMap(gpu_ctx, "f32", *maps["f32"])
    A, B = _tracker(gpu_ctx, w, h, use_graph, cal), _tracker(gpu_ctx, w, h, use_graph, cal)
    rng = np.random.default_rng(4)
    for f in range(nframes):
        if f == 2:
            A.setRectification(rm)
        if f == 3:
            A.setRectification(None)
        if f == 0:
            k, p, hp = EMPTY, EMPTY, None
        else:
            k, p, hp = _points(w, h, flow, f - 1, rng, 1.0)
        _same_frame(A, B, A.trackFrame(raw[f], k, p, hp), B.trackFrame(fed_b[f], k, p, hp), len(k), "frame %d" % f)
    for t in (A, B):
        t.close()
    rm.close()


@pytest.mark.parametrize("look_ahead", [False, True])
def test_lockstep_tracker_rectifies_in_its_enqueue(gpu_ctx, look_ahead):
    """batch 4, n_active 3, raw frames: through trackFrame, and through upload -> prepare -> trackFrameBegin / End with the frames to
    come enqueued between the halves; each item == a single tracker without rectification on remap_ref(raw)"""
    w, h, batch, na, n_max, nframes = 376, 240, 4, 3, 400, 5
    seqs = [_sequence(w, h, nframes, seed=60 + b) for b in range(na)]
    maps = _maps("euroc", w, h)
    rect = [[R.remap(f, "f32", *maps["f32"]) for f in seqs[b][0]] for b in range(na)]
    cal = ov2slam_amd.CameraCalibration(gpu_ctx, "pinhole", *K_EUROC)
    rm = ov2slam_amd.RectifyMap(gpu_ctx, "fixed", *maps["fixed"])
    bt = ov2slam_amd.LockstepTracker(gpu_ctx, batch, w, h, fclahe_val=CLIP, nbmaxkps=n_max)
    bt.setCalibration(cal)
    bt.setRectification(rm)
    singles = [_tracker(gpu_ctx, w, h, False, cal, n_max=n_max) for _ in range(na)]
    rngs = [np.random.default_rng(200 + b) for b in range(na)]

    def fill(f):
        for b in range(na):
            bt.image_buffers[f % 3][b][:, :w] = seqs[b][0][f]

    def ahead(f):
        if f + 2 < nframes:
            bt.upload((f + 2) % 3, na)
        if f + 1 < nframes:
            bt.prepare((f + 1) % 3, na)

    if look_ahead:
        for f in range(3):
            fill(f)
        bt.upload(0, na); bt.prepare(0, na); bt.upload(1, na)
        with pytest.raises(ov2slam_amd.Ov2Error):
            bt.setRectification(None)                                    # a prepared frame waits: between steps only
    for f in range(nframes):
        per = [(EMPTY, EMPTY, np.zeros(0, np.uint8)) if f == 0 else _points(w, h, seqs[b][1], f - 1, rngs[b], 1.0, bad_frac=0.2) for b in range(na)]
        kps = np.zeros((batch, n_max, 2), np.float32); pri = np.zeros((batch, n_max, 2), np.float32)
        hp = np.zeros((batch, n_max), np.uint8); n = np.zeros(na, np.int32)
        for b, (k, p, hq) in enumerate(per):
            n[b] = len(k); kps[b, :len(k)] = k; pri[b, :len(k)] = p; hp[b, :len(k)] = hq
        if look_ahead:
            imgs = [bt.image_buffers[f % 3][b] for b in range(na)]
            if f == 0:
                ahead(f)
                out, st, p3p = bt.trackFrame(imgs, kps, pri, hp, n)
            else:
                bt.trackFrameBegin(imgs, kps, pri, hp, n)
                ahead(f)
                out, st, p3p = bt.trackFrameEnd()
        else:
            out, st, p3p = bt.trackFrame([seqs[b][0][f] for b in range(na)], kps, pri, hp, n)
        pts = np.zeros((na, n_max, 2), np.float32)
        grid = synth.grid_keypoints(w, h, 35, np.random.default_rng(f))
        pts[:, :len(grid)] = grid
        bdesc, bvalid = bt.describeBRIEF(na, pts, np.full(na, len(grid), np.int32))
        for b in range(na):
            k, p, hq = per[b]
            m = len(k)
            so, ss, sp = singles[b].trackFrame(rect[b][f], k, p, hq if m else None)
            assert np.array_equal(_bits(out[b, :m]), _bits(so)) and np.array_equal(st[b, :m], ss) and bool(p3p[b]) == sp, "frame %d item %d" % (f, b)
            for lvl in (0, 2):
                assert np.array_equal(bt.cur_item(b).download(lvl)[0], singles[b].cur_pyr.download(lvl)[0]), "frame %d item %d level %d" % (f, b, lvl)
            sd, sv = singles[b].describeBRIEF(grid)
            assert np.array_equal(bdesc[b, :len(grid)], sd) and np.array_equal(bvalid[b, :len(grid)], sv), "frame %d item %d describeBRIEF" % (f, b)
            if m:
                (bu, bb), (su, sb) = bt.lastKeypoints(b, m), singles[b].lastKeypoints(m)
                assert np.array_equal(_bits(bu), _bits(su)) and np.array_equal(bb.view(np.uint64), sb.view(np.uint64))
        if look_ahead and f + 3 < nframes:
            fill(f + 3)                                                   # staging set f % 3 is free again
    bt.setRectification(None)                                             # between steps: accepted
    for t in singles:
        t.close()
    bt.close()
    rm.close()


@pytest.mark.parametrize("use_clahe", [True, False])
@pytest.mark.parametrize("n_items", [1, 3])
def test_pyr_build_rect(gpu_ctx, n_items, use_clahe):
    w, h = 376, 240
    maps = _maps("wild", w, h)
    raws = [np.ascontiguousarray(synth.frame_pair(w, h, seed=70 + b)[0]) for b in range(n_items)]
    rect = [R.remap(r, "f32", *maps["f32"]) for r in raws]
    rm = ov2slam_amd.RectifyMap(gpu_ctx, "f32", *maps["f32"])
    P = ov2slam_amd.Pyramid(gpu_ctx, w, h, 9, 3, batch=n_items)
    Q = ov2slam_amd.Pyramid(gpu_ctx, w, h, 9, 3, batch=n_items)
    strided = [_strided(r, w + 24, SRC_CANARY)[:, :w] for r in raws]
    P.build_rect(rm, strided, use_clahe=use_clahe, clip_limit=CLIP)
    if n_items == 1:
        Q.build_clahe(rect[0], CLIP, w // 50, h // 50) if use_clahe else Q.build(rect[0])
    else:
        Q.build_clahe_batch(rect, CLIP if use_clahe else -1.0, w // 50, h // 50)
    for b in range(n_items):
        for lvl in range(P.levels):
            assert np.array_equal(P.download(lvl, b, padded=True)[0], Q.download(lvl, b, padded=True)[0]), (b, lvl)
    wrong = ov2slam_amd.Pyramid(gpu_ctx, w + 2, h, 9, 3)
    with pytest.raises(ov2slam_amd.Ov2Error) as e:
        wrong.build_rect(rm, [np.zeros((h, w + 2), np.uint8)])            # map and pyramid differ in size
    assert e.value.code == L.OV2_EINVAL
    for p in (P, Q, wrong):
        p.close()
    rm.close()


def test_stereo_match_on_device_rectified_pair(gpu_ctx):
    """ov2_stereo_match on (the rectifying tracker's left pyramid, the right pyramid of ov2_pyr_build_rect_h) == the same on inputs
    rectified by remap_ref"""
    w, h = 376, 240
    left, right, _ = synth.frame_pair(w, h, seed=9, shift=(-7.0, 0.0), theta=0.0)
    maps = _maps("euroc", w, h)
    rl, rr = R.remap(left, "f32", *maps["f32"]), R.remap(right, "f32", *maps["f32"])
    cal = ov2slam_amd.CameraCalibration(gpu_ctx, "pinhole", *K_EUROC)
    rm = cal.setRectifyMaps("f32", *maps["f32"])
    assert np.array_equal(cal.rectifyImage(left), rl)
    A, B = _tracker(gpu_ctx, w, h, True, cal, rm), _tracker(gpu_ctx, w, h, True, cal)
    A.trackFrame(left, EMPTY, EMPTY, None); B.trackFrame(rl, EMPTY, EMPTY, None)
    Pa = ov2slam_amd.Pyramid(gpu_ctx, w, h, 9, 3).build_rect(rm, right, clip_limit=CLIP)
    Pb = ov2slam_amd.Pyramid(gpu_ctx, w, h, 9, 3).build_clahe(rr, CLIP, w // 50, h // 50)
    kps = synth.grid_keypoints(w, h, 35, np.random.default_rng(2))
    ftrk = ov2slam_amd.FeatureTracker(gpu_ctx, 30, 0.01)
    hp = np.zeros(len(kps), np.uint8)
    oka, ra = stereo.stereo_match_arrays(ftrk, A.cur_pyr, Pa, kps, kps, kps, hp, cal, rect=True)
    okb, rb = stereo.stereo_match_arrays(ftrk, B.cur_pyr, Pb, kps, kps, kps, hp, cal, rect=True)
    assert np.array_equal(oka, okb) and np.array_equal(_bits(ra), _bits(rb)) and oka.any()
    for o in (A, B, Pa, Pb):
        o.close()
    rm.close()


def _wr(f, a):
    b = np.ascontiguousarray(a).tobytes()
    f.write(struct.pack("<q", len(b))); f.write(b)


def _rd(f, dt):
    (n,) = struct.unpack("<q", f.read(8))
    return np.frombuffer(f.read(n), dt).copy()


def test_cpp_adapter_returns_the_same_bytes(gpu_ctx, tmp_path):
    """tests/cpp/rectify_run.cpp: CameraCalibration::setUndistMaps / rectifyImage and FrameTracker::setRectification of
    ov2slam_amd/host, executed on both map forms"""
    exe = tmp_path / "rectify_run"
    libdir = os.path.join(ROOT, "ov2slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "rectify_run.cpp"),
                           "-o", str(exe), "-L", libdir, "-lov2slam_hip", "-Wl,-rpath," + libdir])
    img = _image("noise121x99")
    h, w = img.shape
    ref = _ref("noise121x99", "wild")
    sstride, dstride = w + 11, _up16(w)
    for form, code in (("f32", L.OV2_MAP_F32), ("fixed", L.OV2_MAP_FIXED)):
        m1, m2 = _maps("wild", w, h)[form]
        case, res = tmp_path / ("case_%s.bin" % form), tmp_path / ("res_%s.bin" % form)
        with open(case, "wb") as f:
            _wr(f, np.array([w, h, code, sstride, dstride], np.int32)); _wr(f, m1); _wr(f, m2); _wr(f, _strided(img, sstride, SRC_CANARY))
        r = subprocess.run([str(exe), str(case), str(res)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        with open(res, "rb") as f:
            rect, inplace, lvl0 = _rd(f, np.uint8).reshape(h, dstride), _rd(f, np.uint8).reshape(h, sstride), _rd(f, np.uint8).reshape(h, w)
        assert np.array_equal(rect[:, :w], ref) and (rect[:, w:] == 0xA5).all(), form
        assert np.array_equal(inplace[:, :w], ref) and (inplace[:, w:] == SRC_CANARY).all(), form
        assert np.array_equal(lvl0, ref), form
