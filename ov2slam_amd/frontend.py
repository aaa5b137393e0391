"""Host-side mirror of the reference's front-end operator interface, on top of the
C ABI (include/ov2slam_hip.h).  Names, argument meaning and failure behaviour follow
/root/reference/include/feature_tracker.hpp and feature_extractor.hpp so that the
parity tests read like calls into the reference:

    reference (C++ / OpenCV)                              here
    ----------------------------------------------------  ---------------------------------
    cv::buildOpticalFlowPyramid(img, pyr, win, lvl)       Pyramid(ctx, w, h, win, lvl).build(img)
    FeatureTracker::fbKltTracking(prevpyr, curpyr, ...)   FeatureTracker.fbKltTracking(...)
    FeatureExtractor::detectGridFAST(im, cell, kps, roi)  FeatureExtractor.detectGridFAST(...)
    FeatureExtractor::detectSingleScale(im, cell, ...)    FeatureExtractor.detectSingleScale(...)

numpy arrays are the host buffers; nothing here computes on the CPU.
"""
import ctypes as C
import weakref

import numpy as np

from . import _lib as L


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Context:
    """One HIP stream + scratch (ov2_ctx).  One per calling thread."""

    def __init__(self, device=0, stream=None):
        self.lib = L.load()
        h = C.c_void_p()
        if stream is None:
            L.check(self.lib.ov2_ctx_create(device, C.byref(h)))
        else:
            L.check(self.lib.ov2_ctx_create_on_stream(device, C.c_void_p(stream), C.byref(h)))
        self.h = h
        self.device = device
        # objects that hold device memory / streams of this context: closed before the context itself
        self._children = weakref.WeakSet()

    def sync(self):
        L.check(self.lib.ov2_ctx_sync(self.h))

    def set_option(self, option, value):
        """ov2_ctx_set_option, e.g. (L.OV2_OPT_SOBEL_DY_ORDER, L.OV2_SOBEL_DY_EXACT_SUM)."""
        L.check(self.lib.ov2_ctx_set_option(self.h, int(option), int(value)))

    def get_option(self, option):
        v = C.c_int(0)
        L.check(self.lib.ov2_ctx_get_option(self.h, int(option), C.byref(v)))
        return v.value

    def options(self, **kw):
        """Context manager: pin kernel paths for a block (tests, A/B runs), e.g. ctx.options(lk_impl=L.OV2_LK_IMPL_LANE3);
        names are the OV2_OPT_* suffixes in lower case.  The previous values come back on exit."""
        import contextlib

        @contextlib.contextmanager
        def _cm():
            ids = {k: getattr(L, "OV2_OPT_" + k.upper()) for k in kw}
            old = {k: self.get_option(ids[k]) for k in kw}
            try:
                for k, v in kw.items():
                    self.set_option(ids[k], v)
                yield self
            finally:
                for k, v in old.items():
                    self.set_option(ids[k], v)
        return _cm()

    def set_brief_pattern(self, pairs):
        """ov2_brief_set_pattern: the BRIEF test pairs of this context's describeBRIEF calls, (256, 4) int8 rows {ay, ax, by, bx}
        with offsets in [-24, 24] (e.g. OpenCV's table, tests/golden/brief_pattern_opencv.npy); None restores the built-in table."""
        if pairs is None:
            L.check(self.lib.ov2_brief_set_pattern(self.h, None))
            return
        a = np.asarray(pairs)
        if a.shape != (256, 4):
            raise ValueError("a BRIEF pattern is 256 x 4 offsets, got shape %s" % (a.shape,))
        if np.any(a < -24) or np.any(a > 24):      # (also checked by the library; int8 conversion would wrap first)
            raise ValueError("BRIEF pattern offsets must lie in [-24, 24]")
        a = np.ascontiguousarray(a, np.int8)
        L.check(self.lib.ov2_brief_set_pattern(self.h, _ptr(a)))

    def brief_pattern(self):
        """-> (256, 4) int8: the test pairs describeBRIEF uses on this context"""
        a = np.zeros((256, 4), np.int8)
        L.check(self.lib.ov2_brief_get_pattern(self.h, _ptr(a)))
        return a

    @property
    def stream(self):
        return self.lib.ov2_ctx_stream(self.h)

    def close(self):
        if getattr(self, "h", None):
            for c in list(self._children):
                c.close()
            self.lib.ov2_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Pyramid:
    """Device-resident result of cv::buildOpticalFlowPyramid (image + Scharr
    derivative per level, padded by `win`), for `batch` images of equal size."""

    def __init__(self, ctx, w, h, win=9, max_level=3, batch=1):
        self.ctx, self.lib = ctx, ctx.lib
        self.w, self.h, self.win, self.max_level, self.batch = w, h, win, max_level, batch
        hp = C.c_void_p()
        L.check(self.lib.ov2_pyr_create(ctx.h, w, h, win, max_level, batch, C.byref(hp)))
        self.h_pyr = hp
        ctx._children.add(self)

    @property
    def levels(self):
        return self.lib.ov2_pyr_levels(self.h_pyr)

    def level_size(self, level):
        w, h = C.c_int(), C.c_int()
        L.check(self.lib.ov2_pyr_level_size(self.h_pyr, level, C.byref(w), C.byref(h)))
        return w.value, h.value

    def build(self, img):
        """img: (h,w) or (batch,h,w) uint8 numpy array (host).  Asynchronous."""
        img = np.ascontiguousarray(img, dtype=np.uint8)
        if img.ndim == 2:
            img = img[None]
        assert img.shape == (self.batch, self.h, self.w), img.shape
        self._keep = img
        L.check(self.lib.ov2_pyr_build_h(self.ctx.h, self.h_pyr, _ptr(img), self.w, self.w * self.h))
        return self

    def build_from_device(self, dev_ptr, stride=None, batch_stride=None):
        stride = stride or self.w
        batch_stride = batch_stride or stride * self.h
        L.check(self.lib.ov2_pyr_build_d(self.ctx.h, self.h_pyr, C.c_void_p(dev_ptr), stride, batch_stride))
        return self

    def build_clahe(self, img, clip_limit, tiles_x, tiles_y):
        """preprocessImage from a host image (batch 1): CLAHE written straight into level 0 + coarser levels."""
        img = np.ascontiguousarray(img, dtype=np.uint8)
        assert img.shape == (self.h, self.w) and self.batch == 1
        self._keep = img
        L.check(self.lib.ov2_pyr_build_clahe_h(self.ctx.h, self.h_pyr, _ptr(img), self.w, float(clip_limit), int(tiles_x), int(tiles_y)))
        return self

    def build_clahe_batch(self, imgs, clip_limit, tiles_x, tiles_y):
        """preprocessImage of len(imgs) host images into items [0, len(imgs)) of this batch pyramid in one enqueue (ov2_pyr_build_clahe_hb);
        clip_limit < 0: no CLAHE"""
        imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in imgs]
        for im in imgs:
            assert im.shape == (self.h, self.w)
        self._keep = imgs
        ptrs = (C.c_void_p * len(imgs))(*[im.ctypes.data for im in imgs])
        L.check(self.lib.ov2_pyr_build_clahe_hb(self.ctx.h, self.h_pyr, len(imgs), ptrs, self.w, float(clip_limit), int(tiles_x), int(tiles_y)))
        return self

    def build_rect(self, rmap, imgs, use_clahe=True, clip_limit=3.0, tiles_x=None, tiles_y=None):
        """The right image(s) of a stereo keyframe from RAW host frames (ov2_pyr_build_rect_h): upload, rectifyImage through `rmap`
        (a RectifyMap), then build_clahe / build_clahe_batch (use_clahe) or build of the rectified frames, into items
        [0, len(imgs)).  imgs: one (h, >= w) uint8 array or a list of them with one common row pitch."""
        if isinstance(imgs, np.ndarray) and imgs.ndim == 2:
            imgs = [imgs]
        imgs = [im if im.dtype == np.uint8 and im.ndim == 2 and im.strides[1] == 1 else np.ascontiguousarray(im, np.uint8) for im in imgs]
        stride = imgs[0].strides[0]
        for im in imgs:
            if im.ndim != 2 or im.shape[0] != self.h or im.shape[1] < self.w or im.strides[0] != stride:
                raise ValueError("frames must be %d rows of >= %d bytes with one common row pitch" % (self.h, self.w))
        self._keep = imgs
        ptrs = (C.c_void_p * len(imgs))(*[im.ctypes.data for im in imgs])
        tx = self.w // 50 if tiles_x is None else int(tiles_x)
        ty = self.h // 50 if tiles_y is None else int(tiles_y)
        L.check(self.lib.ov2_pyr_build_rect_h(self.ctx.h, self.h_pyr, rmap.h_map, len(imgs), ptrs, stride, int(bool(use_clahe)),
                                              float(clip_limit), tx, ty))
        return self

    def build_clahe_from_device(self, dev_ptr, clip_limit, tiles_x, tiles_y, stride=None, batch_stride=None):
        """preprocessImage: CLAHE written straight into level 0, then the coarser levels (one call)."""
        stride = stride or self.w
        batch_stride = batch_stride or stride * self.h
        L.check(self.lib.ov2_pyr_build_clahe_d(self.ctx.h, self.h_pyr, C.c_void_p(dev_ptr), stride, batch_stride,
                                               float(clip_limit), int(tiles_x), int(tiles_y)))
        return self

    def download(self, level, b=0, padded=False):
        w, h = self.level_size(level)
        if padded:
            w, h = w + 2 * self.win, h + 2 * self.win
        img = np.empty((h, w), np.uint8)
        der = np.empty((h, w, 2), np.int16)
        fn = self.lib.ov2_pyr_download_padded if padded else self.lib.ov2_pyr_download
        L.check(fn(self.ctx.h, self.h_pyr, b, level, _ptr(img), _ptr(der)))
        return img, der

    def download_item(self, b=0):
        """item b as it lies in device memory (every level, its borders, the slack between them): a uint8 array of the item stride"""
        raw = np.empty(int(self.lib.ov2_pyr_item_bytes(self.h_pyr)), np.uint8)
        L.check(self.lib.ov2_pyr_download_item(self.ctx.h, self.h_pyr, int(b), _ptr(raw)))
        return raw

    @property
    def algorithmic_bytes(self):
        return self.lib.ov2_pyr_algorithmic_bytes(self.h_pyr)

    def close(self):
        if getattr(self, "h_pyr", None):
            self.lib.ov2_pyr_destroy(self.h_pyr)
            self.h_pyr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RectifyMap:
    """Device form of the pair (undist_map_x_, undist_map_y_) a CameraCalibration holds after setUndistMap / setUndistStereoMap
    (the reference's src/camera_calibration.cpp:92-97, :141-145): ov2_rectmap.  form "f32": map1 = source x, map2 = source y, (h, w)
    float32 each (CV_32FC1); form "fixed": map1 (h, w, 2) int16 = (ix, iy) (CV_16SC2), map2 (h, w) uint16 = b * 32 + a (CV_16UC1).
    Immutable; keep it alive while a tracker uses it."""

    FORMS = {"f32": L.OV2_MAP_F32, "fixed": L.OV2_MAP_FIXED}

    def __init__(self, ctx, form, map1, map2):
        self.ctx, self.lib = ctx, ctx.lib
        f = self.FORMS[form] if isinstance(form, str) else int(form)
        if f == L.OV2_MAP_F32:
            m1 = np.ascontiguousarray(map1, np.float32); m2 = np.ascontiguousarray(map2, np.float32)
            if m1.ndim != 2 or m1.shape != m2.shape:
                raise ValueError("an f32 map is two (h, w) float32 arrays")
        else:
            m1 = np.ascontiguousarray(map1, np.int16); m2 = np.ascontiguousarray(map2, np.uint16)
            if m1.ndim != 3 or m1.shape[2] != 2 or m1.shape[:2] != m2.shape:
                raise ValueError("a fixed-point map is (h, w, 2) int16 + (h, w) uint16")
        self.h, self.w = int(m2.shape[0]), int(m2.shape[1])
        hm = C.c_void_p()
        L.check(self.lib.ov2_rectmap_create(ctx.h, self.w, self.h, f, _ptr(m1), _ptr(m2), C.byref(hm)))
        self.h_map = hm
        ctx._children.add(self)

    def rectify(self, img, out=None):
        """rectifyImage of an (h, >= w) uint8 host image (any row stride) -> the rectified (h, w) image; out: the array to write
        (may be img itself: the reference rectifies in place)"""
        img = img if img.dtype == np.uint8 and img.ndim == 2 and img.strides[1] == 1 else np.ascontiguousarray(img, np.uint8)
        if img.shape[0] != self.h or img.shape[1] < self.w:
            raise ValueError("image shape %s does not match the map's %dx%d" % (img.shape, self.w, self.h))
        if out is None:
            out = np.empty((self.h, self.w), np.uint8)
        if out.dtype != np.uint8 or out.ndim != 2 or out.strides[1] != 1 or out.shape[0] != self.h or out.shape[1] < self.w:
            raise ValueError("out must be an (h, >= w) uint8 array with unit column stride")
        L.check(self.lib.ov2_rectify_h(self.ctx.h, self.h_map, _ptr(img), img.strides[0], _ptr(out), out.strides[0]))
        return out

    def rectify_device(self, src_d, src_pitch, src_item_stride, n_items, dst_d, dst_pitch, dst_item_stride):
        """ov2_rectify_d: device addresses (ints), asynchronous on the context's stream"""
        L.check(self.lib.ov2_rectify_d(self.ctx.h, self.h_map, C.c_void_p(src_d), int(src_pitch), int(src_item_stride), int(n_items),
                                       C.c_void_p(dst_d), int(dst_pitch), int(dst_item_stride)))

    def close(self):
        if getattr(self, "h_map", None):
            self.lib.ov2_rectmap_destroy(self.h_map)
            self.h_map = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CLAHE:
    """Mirror of the cv::CLAHE handle the reference creates at src/ov2slam.cpp:85-89 and applies at
    src/visual_front_end.cpp:1159 / src/mapper.cpp:76:  createCLAHE(clipLimit, tileGridSize).apply(src)."""

    def __init__(self, ctx, clipLimit=3.0, tileGridSize=(15, 9)):
        self.ctx, self.lib = ctx, ctx.lib
        self.clipLimit = float(clipLimit)
        self.tiles_x, self.tiles_y = int(tileGridSize[0]), int(tileGridSize[1])

    def apply(self, src):
        src = np.ascontiguousarray(src, dtype=np.uint8)
        h, w = src.shape
        dst = np.empty_like(src)
        L.check(self.lib.ov2_clahe_h(self.ctx.h, _ptr(src), w, h, w, self.clipLimit, self.tiles_x, self.tiles_y, _ptr(dst), w))
        return dst


class FeatureTracker:
    """Mirror of /root/reference/include/feature_tracker.hpp:36-56.

    FeatureTracker(nmax_iter, fmax_px_precision) stores the KLT convergence criteria
    (cv::TermCriteria(COUNT+EPS, nmax_iter, fmax_px_precision), :39-40)."""

    def __init__(self, ctx, nmax_iter=30, fmax_px_precision=0.01):
        self.ctx, self.lib = ctx, ctx.lib
        self.nmax_iter = int(nmax_iter)
        self.fmax_px_precision = float(np.float32(fmax_px_precision))

    def fbKltTracking(self, vprevpyr, vcurpyr, nwinsize, nbpyrlvl, ferr, fmax_fbklt_dist, vkps, vpriorkps,
                      return_stats=False):
        """src/feature_tracker.cpp:35-137.  vkps / vpriorkps: (n,2) float32.
        Returns (vpriorkps_out, vkpstatus) -- the reference updates vpriorkps in place
        and push_back()s into vkpstatus; with no keypoints it returns untouched
        outputs (:43-46), here an empty status list."""
        kps = np.ascontiguousarray(vkps, dtype=np.float32).reshape(-1, 2)
        pri = np.array(vpriorkps, dtype=np.float32, copy=True).reshape(-1, 2)
        n = kps.shape[0]
        assert pri.shape[0] == n
        status = np.zeros(n, np.uint8)
        stats = (C.c_longlong * 2)(0, 0)
        L.check(self.lib.ov2_fb_klt(self.ctx.h, vprevpyr.h_pyr, vcurpyr.h_pyr, int(nwinsize), int(nbpyrlvl),
                                    self.nmax_iter, self.fmax_px_precision, float(ferr), float(fmax_fbklt_dist),
                                    _ptr(kps), _ptr(pri), n, _ptr(status), stats))
        if return_stats:
            return pri, status.astype(bool), (int(stats[0]), int(stats[1]))
        return pri, status.astype(bool)

    def getLineMinSAD(self, leftpyr, rightpyr, level, pts, nwinsize=7, bgoleft=True):
        """src/feature_tracker.cpp:138-206 for an (n,2) array of points already scaled to `level`
        (the reference passes vleftpyr.at(2 * nklt_pyr_lvl_) and kp.px_ * downpyrcoef, map_manager.cpp:427-431).
        Returns (xprior (n,) float32, -1 = none; l1err (n,) float32)."""
        pts = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 2)
        n = len(pts)
        xp = np.full(n, -1, np.float32); err = np.full(n, 255, np.float32)
        L.check(self.lib.ov2_line_min_sad(self.ctx.h, leftpyr.h_pyr, rightpyr.h_pyr, int(level), int(nwinsize), int(bool(bgoleft)),
                                          _ptr(pts), n, _ptr(xp), _ptr(err)))
        return xp, err

    def calcOpticalFlowPyrLK(self, prevpyr, nextpyr, prevpts, nextpts, nwinsize, maxlevel,
                             flags=L.OV2_LK_USE_INITIAL_FLOW | L.OV2_LK_GET_MIN_EIGENVALS):
        """One cv::calcOpticalFlowPyrLK call (src/feature_tracker.cpp:66-69)."""
        p0 = np.ascontiguousarray(prevpts, dtype=np.float32).reshape(-1, 2)
        p1 = np.array(nextpts, dtype=np.float32, copy=True).reshape(-1, 2)
        n = p0.shape[0]
        status = np.zeros(n, np.uint8)
        err = np.zeros(n, np.float32)
        iters = np.zeros(n, np.int32)
        L.check(self.lib.ov2_lk_track(self.ctx.h, prevpyr.h_pyr, nextpyr.h_pyr, int(nwinsize), int(maxlevel),
                                      self.nmax_iter, self.fmax_px_precision, int(flags),
                                      _ptr(p0), _ptr(p1), n, _ptr(status), _ptr(err), _ptr(iters)))
        return p1, status, err, iters


class _PyrView:
    """Borrowed ov2_pyr handle (owned by a Tracker): usable wherever a Pyramid is expected."""

    def __init__(self, ctx, h_pyr, w, h, win):
        self.ctx, self.lib, self.h_pyr, self.w, self.h, self.win, self.batch = ctx, ctx.lib, h_pyr, w, h, win, 1

    levels = Pyramid.levels
    level_size = Pyramid.level_size
    download = Pyramid.download
    download_item = Pyramid.download_item


class VisualFrontEndTracker:
    """The per-frame GPU half of the reference's VisualFrontEnd (src/visual_front_end.cpp): it owns prev_pyr_ / cur_pyr_
    and performs preprocessImage (:1143-1177) + kltTracking (:132-275) per frame -- one H2D of the frame, one H2D of the
    keypoint block, ONE LK launch for both fbKltTracking calls and the retry of lost prior tracks, one D2H, one sync
    (ov2_tracker_*).  Parameters are the SlamParams fields of the same names."""

    def __init__(self, ctx, w, h, nklt_win_size=9, nklt_pyr_lvl=3, nmax_iter=30, fmax_px_precision=0.01, nklt_err=30.0,
                 fmax_fbklt_dist=0.5, use_clahe=True, fclahe_val=3.0, nbmaxkps=512, use_graph=True, prior_pyr_lvl=1):
        self.ctx, self.lib = ctx, ctx.lib
        self.w, self.h, self.win = int(w), int(h), int(nklt_win_size)
        cfg = L.TrackerConfig(self.w, self.h, self.win, int(nklt_pyr_lvl), int(prior_pyr_lvl), int(nmax_iter),
                              float(np.float32(fmax_px_precision)), float(nklt_err), float(fmax_fbklt_dist),
                              int(bool(use_clahe)), float(fclahe_val), self.w // 50, self.h // 50, int(nbmaxkps),
                              int(bool(use_graph)))
        ht = C.c_void_p()
        L.check(self.lib.ov2_tracker_create(ctx.h, C.byref(cfg), C.byref(ht)))
        self.h_trk = ht
        ctx._children.add(self)
        self.nbmaxkps = int(nbmaxkps)
        stride = C.c_int()
        ptr = self.lib.ov2_tracker_image_buffer(ht, C.byref(stride))
        self.stride = stride.value
        # numpy view of the pinned staging image: write the next frame here to skip the host-side copy
        self.image_buffer = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(self.h, self.stride))

    def _pts(self, vkps, vpriors, vhasprior):
        kps = np.ascontiguousarray(vkps, dtype=np.float32).reshape(-1, 2)
        pri = np.ascontiguousarray(vpriors, dtype=np.float32).reshape(-1, 2)
        n = len(kps)
        if len(pri) != n:
            raise ValueError("vkps and vpriors differ in length")
        hp = None if vhasprior is None else np.ascontiguousarray(vhasprior, dtype=np.uint8).reshape(-1)
        if hp is not None and len(hp) != n:
            raise ValueError("vhasprior has %d entries for %d keypoints" % (len(hp), n))
        return kps, pri, hp, n

    def _img(self, img_raw):
        img = img_raw if img_raw is self.image_buffer else np.ascontiguousarray(img_raw, dtype=np.uint8)
        if img.ndim != 2 or img.shape[0] != self.h or img.shape[1] < self.w:       # the C side reads h rows of w bytes
            raise ValueError("image shape %s does not match the tracker's %dx%d" % (img.shape, self.w, self.h))
        return img

    def preprocessImage(self, img_raw):
        """Asynchronous (returns after the enqueue)."""
        img = self._img(img_raw)
        L.check(self.lib.ov2_tracker_preprocess(self.h_trk, _ptr(img), img.strides[0]))

    def kltTracking(self, vkps, vpriors, vhasprior, klt_use_prior=True):
        """-> (tracked px (n,2), status bits (n,) uint8 [bit0 tracked, bit1 re-tracked on the full pyramid], bp3preq)."""
        kps, pri, hp, n = self._pts(vkps, vpriors, vhasprior)
        out = np.zeros((n, 2), np.float32); st = np.zeros(n, np.uint8); p3p = C.c_int(0)
        L.check(self.lib.ov2_tracker_klt(self.h_trk, _ptr(kps), _ptr(pri), _ptr(hp), n, int(bool(klt_use_prior)),
                                         _ptr(out), _ptr(st), C.byref(p3p)))
        return out, st, bool(p3p.value)

    def trackFrame(self, img_raw, vkps, vpriors, vhasprior, klt_use_prior=True):
        """preprocessImage + kltTracking in one enqueue (graph replay when enabled)."""
        img = self._img(img_raw)
        kps, pri, hp, n = self._pts(vkps, vpriors, vhasprior)
        out = np.zeros((n, 2), np.float32); st = np.zeros(n, np.uint8); p3p = C.c_int(0)
        L.check(self.lib.ov2_tracker_track_frame(self.h_trk, _ptr(img), img.strides[0], _ptr(kps), _ptr(pri), _ptr(hp), n,
                                                 int(bool(klt_use_prior)), _ptr(out), _ptr(st), C.byref(p3p)))
        return out, st, bool(p3p.value)

    def describeBRIEF(self, vpts):
        """FeatureExtractor::describeBRIEF on the RAW current frame (the image of the last preprocessImage / trackFrame, before
        CLAHE; already on the device) -> (desc (n, 32) uint8, valid (n,) bool)"""
        pts = np.ascontiguousarray(vpts, dtype=np.float32).reshape(-1, 2)
        n = len(pts)
        desc = np.zeros((n, L.OV2_BRIEF_BYTES), np.uint8); valid = np.zeros(n, np.uint8)
        L.check(self.lib.ov2_tracker_describe_brief(self.h_trk, _ptr(pts), n, _ptr(desc), _ptr(valid)))
        return desc, valid.astype(bool)

    def setCalibration(self, calib):
        """calib: CameraCalibration.  From now on every kltTracking / trackFrame also computes Frame::computeKeypoint (undistorted
        pixel + bearing vector) of its output positions in the same enqueue: lastKeypoints().  Call right after construction."""
        L.check(self.lib.ov2_tracker_set_calibration(self.h_trk, calib.model, _ptr(calib.K), _ptr(calib.D) if calib.D is not None else None,
                                                     0 if calib.D is None else len(calib.D), _ptr(calib.iK)))

    def setRectification(self, rmap):
        """rmap: RectifyMap or None.  From now on preprocessImage / trackFrame take RAW frames and run CameraCalibration::rectifyImage
        inside the same enqueue; describeBRIEF and the detectors on cur_pyr then see the rectified frame.  None switches it off."""
        L.check(self.lib.ov2_tracker_set_rectification(self.h_trk, rmap.h_map if rmap is not None else None))
        self._rmap = rmap                                    # the map must outlive its use by the tracker

    def lastKeypoints(self, n, want_bv=True):
        """(unpx (n,2) float32, bv (n,3) float64 or None) of the n keypoints of the last kltTracking / trackFrame call."""
        unpx = np.empty((n, 2), np.float32)
        bv = np.empty((n, 3), np.float64) if want_bv else None
        L.check(self.lib.ov2_tracker_last_keypoints(self.h_trk, int(n), _ptr(unpx), _ptr(bv) if want_bv else None))
        return unpx, bv

    @property
    def cur_pyr(self):
        return _PyrView(self.ctx, C.c_void_p(self.lib.ov2_tracker_cur_pyr(self.h_trk)), self.w, self.h, self.win)

    @property
    def prev_pyr(self):
        return _PyrView(self.ctx, C.c_void_p(self.lib.ov2_tracker_prev_pyr(self.h_trk)), self.w, self.h, self.win)

    @property
    def uses_graph(self):
        return bool(self.lib.ov2_tracker_uses_graph(self.h_trk))

    def close(self):
        if getattr(self, "h_trk", None):
            self.image_buffer = None
            self.lib.ov2_tracker_destroy(self.h_trk)
            self.h_trk = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LockstepTracker:
    """`batch` camera streams in lock-step (ov2_btracker_*, csrc/trackb.hip): the offline batch-of-sequences form of
    VisualFrontEndTracker.  Every call advances items [0, n_active) by one frame with ONE enqueue over all of them; results per
    item are bit-identical to a VisualFrontEndTracker fed the same frames and keypoints.  Point arrays are (batch, n_max, 2) with
    n[b] valid rows per item."""

    def __init__(self, ctx, batch, w, h, nklt_win_size=9, nklt_pyr_lvl=3, nmax_iter=30, fmax_px_precision=0.01, nklt_err=30.0,
                 fmax_fbklt_dist=0.5, use_clahe=True, fclahe_val=3.0, nbmaxkps=512, prior_pyr_lvl=1):
        self.ctx, self.lib = ctx, ctx.lib
        self.batch, self.w, self.h, self.win, self.n_max = int(batch), int(w), int(h), int(nklt_win_size), int(nbmaxkps)
        cfg = L.TrackerConfig(self.w, self.h, self.win, int(nklt_pyr_lvl), int(prior_pyr_lvl), int(nmax_iter),
                              float(np.float32(fmax_px_precision)), float(nklt_err), float(fmax_fbklt_dist),
                              int(bool(use_clahe)), float(fclahe_val), self.w // 50, self.h // 50, self.n_max, 0)
        ht = C.c_void_p()
        L.check(self.lib.ov2_btracker_create(ctx.h, C.byref(cfg), self.batch, C.byref(ht)))
        self.h_trk = ht
        ctx._children.add(self)
        stride = C.c_int()
        self.image_buffers = []                       # [which][item] -> numpy view of the pinned slot
        for which in range(3):
            row = []
            for b in range(self.batch):
                ptr = self.lib.ov2_btracker_image_buffer(ht, which, b, C.byref(stride))
                row.append(np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(self.h, stride.value)))
            self.image_buffers.append(row)
        self.stride = stride.value

    def setCalibration(self, calib):
        L.check(self.lib.ov2_btracker_set_calibration(self.h_trk, calib.model, _ptr(calib.K), _ptr(calib.D) if calib.D is not None else None,
                                                      0 if calib.D is None else len(calib.D), _ptr(calib.iK)))

    def setRectification(self, rmap):
        """rmap: RectifyMap or None: the frames of trackFrame / upload / prepare are RAW from now on (rectified in the same enqueue,
        before CLAHE).  Between steps only."""
        L.check(self.lib.ov2_btracker_set_rectification(self.h_trk, rmap.h_map if rmap is not None else None))
        self._rmap = rmap

    def upload(self, which, n_active):
        """start the H2D of staging set `which` (already filled through image_buffers[which]) on the copy stream"""
        L.check(self.lib.ov2_btracker_upload(self.h_trk, int(which), int(n_active)))

    def prepare(self, which, n_active):
        """preprocessImage of staging set `which` for the NEXT trackFrame, on the tracker's prep stream"""
        L.check(self.lib.ov2_btracker_prepare(self.h_trk, int(which), int(n_active)))

    def _frames(self, imgs):
        """the frames of a step -> (contiguous list, common row pitch, pointer array); refuses a wrong shape or mixed pitches"""
        imgs = [im if im.dtype == np.uint8 and im.strides[1] == 1 else np.ascontiguousarray(im, np.uint8) for im in imgs]
        stride = imgs[0].strides[0]
        for im in imgs:
            if im.ndim != 2 or im.shape[0] != self.h or im.shape[1] < self.w or im.strides[0] != stride:
                raise ValueError("frames must be %d rows of >= %d bytes with one common row pitch" % (self.h, self.w))
        return imgs, stride, (C.c_void_p * len(imgs))(*[im.ctypes.data for im in imgs])

    def _outputs(self, na):
        """the result arrays of a step: out (batch, n_max, 2), status bits (batch, n_max), p3p_req (na,)"""
        return np.zeros((self.batch, self.n_max, 2), np.float32), np.zeros((self.batch, self.n_max), np.uint8), np.zeros(na, np.int32)

    def trackFrame(self, imgs, kps, pri, hasprior, n, klt_use_prior=True):
        """imgs: list of n_active (h, >=w) uint8 arrays of one row pitch (or pinned slots of one staging set); kps / pri:
        (batch, n_max, 2) float32; hasprior: (batch, n_max) uint8 or None; n: per-item counts (len n_active).
        -> (out (batch, n_max, 2), status bits (batch, n_max), p3p_req (n_active,) bool)"""
        na = len(imgs)
        imgs, stride, ptrs = self._frames(imgs)
        kps = np.ascontiguousarray(kps, np.float32).reshape(self.batch, self.n_max, 2)
        pri = np.ascontiguousarray(pri, np.float32).reshape(self.batch, self.n_max, 2)
        hp = None if hasprior is None else np.ascontiguousarray(hasprior, np.uint8).reshape(self.batch, self.n_max)
        nn = np.ascontiguousarray(n, np.int32)
        if len(nn) != na:
            raise ValueError("one keypoint count per active item")
        out, st, p3p = self._outputs(na)
        L.check(self.lib.ov2_btracker_track_frame(self.h_trk, na, ptrs, stride, _ptr(kps), _ptr(pri), _ptr(hp), _ptr(nn),
                                                  int(bool(klt_use_prior)), _ptr(out), _ptr(st), _ptr(p3p)))
        return out, st, p3p.astype(bool)

    def trackFrameBegin(self, imgs, kps, pri, hasprior, n, klt_use_prior=True):
        """first half of trackFrame: enqueue the step and return (upload / prepare of the frames to come go between the halves)"""
        na = len(imgs)
        imgs, stride, ptrs = self._frames(imgs)
        kps = np.ascontiguousarray(kps, np.float32).reshape(self.batch, self.n_max, 2)
        pri = np.ascontiguousarray(pri, np.float32).reshape(self.batch, self.n_max, 2)
        hp = None if hasprior is None else np.ascontiguousarray(hasprior, np.uint8).reshape(self.batch, self.n_max)
        nn = np.ascontiguousarray(n, np.int32)
        self._pending = (imgs, kps, pri, hp, nn)                                  # (kps / hasprior are re-read by trackFrameEnd: keep them alive)
        L.check(self.lib.ov2_btracker_track_frame_begin(self.h_trk, na, ptrs, stride, _ptr(kps), _ptr(pri), _ptr(hp), _ptr(nn), int(bool(klt_use_prior))))

    def trackFrameEnd(self):
        """second half: wait, results, p3p rule -> (out, status bits, p3p_req) as trackFrame"""
        na = len(self._pending[0])
        out, st, p3p = self._outputs(na)
        L.check(self.lib.ov2_btracker_track_frame_end(self.h_trk, _ptr(out), _ptr(st), _ptr(p3p)))
        self._pending = None
        return out, st, p3p.astype(bool)

    def _map_args(self, imgs, kps, wpt, is3d, Tcw, n):
        na = len(imgs)
        imgs, stride, ptrs = self._frames(imgs)
        kps = np.ascontiguousarray(kps, np.float32).reshape(self.batch, self.n_max, 2)
        wpt = np.ascontiguousarray(wpt, np.float64).reshape(self.batch, self.n_max, 3)
        is3d = np.ascontiguousarray(is3d, np.uint8).reshape(self.batch, self.n_max)
        Tcw = np.ascontiguousarray(Tcw, np.float64).reshape(-1, 7)
        nn = np.ascontiguousarray(n, np.int32)
        if len(nn) != na or len(Tcw) < na:
            raise ValueError("one keypoint count and one predicted pose per active item")
        return na, imgs, stride, ptrs, kps, wpt, is3d, Tcw, nn

    def trackFrameMap(self, imgs, kps, wpt, is3d, Tcw, n, klt_use_prior=True):
        """trackFrame with the priors derived on the device (ov2_btracker_track_frame_map): wpt (batch, n_max, 3) float64 map points,
        is3d (batch, n_max) uint8, Tcw (>= n_active, 7) the predicted poses [t q], already inverted.  Needs setCalibration.
        -> (out, status bits, p3p_req) as trackFrame; lastPriors returns the priors that were used."""
        na, imgs, stride, ptrs, kps, wpt, is3d, Tcw, nn = self._map_args(imgs, kps, wpt, is3d, Tcw, n)
        out, st, p3p = self._outputs(na)
        L.check(self.lib.ov2_btracker_track_frame_map(self.h_trk, na, ptrs, stride, _ptr(kps), _ptr(wpt), _ptr(is3d), _ptr(Tcw), _ptr(nn),
                                                      int(bool(klt_use_prior)), _ptr(out), _ptr(st), _ptr(p3p)))
        return out, st, p3p.astype(bool)

    track_frame_map = trackFrameMap

    def trackFrameMapBegin(self, imgs, kps, wpt, is3d, Tcw, n, klt_use_prior=True):
        """first half of trackFrameMap; trackFrameEnd finishes it"""
        na, imgs, stride, ptrs, kps, wpt, is3d, Tcw, nn = self._map_args(imgs, kps, wpt, is3d, Tcw, n)
        self._pending = (imgs, kps, wpt, is3d, nn)                                # (kps is re-read by trackFrameEnd: keep it alive)
        L.check(self.lib.ov2_btracker_track_frame_map_begin(self.h_trk, na, ptrs, stride, _ptr(kps), _ptr(wpt), _ptr(is3d), _ptr(Tcw),
                                                            _ptr(nn), int(bool(klt_use_prior))))

    def _pose_args(self, na, nn, params, Twc, p3p_req, seed, scale, dop3p, n_rows):
        from . import pose as _pose
        fp = L.FramePoseParams()
        fp.pose, fp.dop3p, fp.n_rows = _pose._as_pose_params(params), int(bool(dop3p)), int(n_rows)
        self._pose_rows = max(0, int(n_rows))                                     # (the room lastPoseInputs gives the table)
        Twc = np.ascontiguousarray(Twc, np.float64).reshape(-1, 7)
        req = np.ascontiguousarray(p3p_req, np.uint8).reshape(-1)
        seed = np.ascontiguousarray(seed, np.uint64).reshape(-1)
        sc = None if scale is None else np.ascontiguousarray(scale, np.int32).reshape(self.batch, self.n_max)
        if len(Twc) < na or len(req) < na or len(seed) < na:
            raise ValueError("one pose, one p3p request and one seed per active item")
        fi = L.FramePoseInput()
        fi.Twc_h = Twc.ctypes.data_as(C.POINTER(C.c_double))
        fi.scale_h = None if sc is None else sc.ctypes.data_as(C.POINTER(C.c_int))
        fi.p3p_req_h = req.ctypes.data_as(C.POINTER(C.c_uint8))
        fi.seed_h = seed.ctypes.data_as(C.POINTER(C.c_ulonglong))
        return fp, fi, (Twc, req, seed, sc)

    def _pose_results(self, na, nn):
        R = (L.PoseResult * max(1, na))()
        removed = np.zeros((max(1, na), self.n_max), np.uint8)
        for b in range(na):
            R[b].removed = removed[b].ctypes.data_as(C.POINTER(C.c_uint8))
        return R, removed

    def _pose_dicts(self, R, removed, nn):
        from . import pose as _pose
        return [_pose._pose_finish(R[b], dict(unpx=removed[b, :int(nn[b])], removed=removed[b])) for b in range(len(nn))]

    def trackFramePose(self, imgs, kps, wpt, is3d, Tcw, n, params, Twc, p3p_req, seed, scale=None, dop3p=False, n_rows=0,
                       klt_use_prior=True):
        """trackFrameMap and the per-frame pose in one enqueue and one synchronisation (ov2_btracker_track_frame_pose).  params: as
        pose.compute_pose takes them; Twc (>= n_active, 7): the predicted poses NOT inverted (Tcw: the same, inverted); p3p_req, seed:
        one per item; scale (batch, n_max) int or None; dop3p, n_rows: SlamParams::dop3p_ and the rows of the table drawn for an item
        that searches.  -> (out, status bits, p3p_req, poses): poses[b] as pose.compute_pose returns it, with removed (n[b],) IN SLOT
        SPACE."""
        na, imgs, stride, ptrs, kps, wpt, is3d, Tcw, nn = self._map_args(imgs, kps, wpt, is3d, Tcw, n)
        fp, fi, keep = self._pose_args(na, nn, params, Twc, p3p_req, seed, scale, dop3p, n_rows)
        out, st, p3p = self._outputs(na)
        R, removed = self._pose_results(na, nn)
        L.check(self.lib.ov2_btracker_track_frame_pose(self.h_trk, na, ptrs, stride, _ptr(kps), _ptr(wpt), _ptr(is3d), _ptr(Tcw), _ptr(nn),
                                                       int(bool(klt_use_prior)), C.byref(fp), C.byref(fi), _ptr(out), _ptr(st), _ptr(p3p), R))
        return out, st, p3p.astype(bool), self._pose_dicts(R, removed, nn)

    def trackFramePoseBegin(self, imgs, kps, wpt, is3d, Tcw, n, params, Twc, p3p_req, seed, scale=None, dop3p=False, n_rows=0,
                            klt_use_prior=True):
        """first half of trackFramePose; trackFramePoseEnd finishes it (trackFrameEnd finishes the tracking half and drops the pose)"""
        na, imgs, stride, ptrs, kps, wpt, is3d, Tcw, nn = self._map_args(imgs, kps, wpt, is3d, Tcw, n)
        fp, fi, keep = self._pose_args(na, nn, params, Twc, p3p_req, seed, scale, dop3p, n_rows)
        L.check(self.lib.ov2_btracker_track_frame_pose_begin(self.h_trk, na, ptrs, stride, _ptr(kps), _ptr(wpt), _ptr(is3d), _ptr(Tcw),
                                                             _ptr(nn), int(bool(klt_use_prior)), C.byref(fp), C.byref(fi)))
        self._pending = (imgs, kps, wpt, is3d, nn)                                # (kps is re-read by the end half: keep it alive)

    def trackFramePoseEnd(self):
        """second half of trackFramePose -> (out, status bits, p3p_req, poses)"""
        nn = self._pending[4]
        na = len(nn)
        out, st, p3p = self._outputs(na)
        R, removed = self._pose_results(na, nn)
        L.check(self.lib.ov2_btracker_track_frame_pose_end(self.h_trk, _ptr(out), _ptr(st), _ptr(p3p), R))
        self._pending = None
        return out, st, p3p.astype(bool), self._pose_dicts(R, removed, nn)

    def lastPoseInputs(self, item):
        """what the last pose step fed the chain for `item` -> (m, slots (m,) int32, samples (rows used, 4) int32)"""
        m, rows = C.c_int(), C.c_int()
        slot = np.zeros(self.n_max, np.int32)
        tab = np.zeros((max(1, self._pose_rows), 4), np.int32)
        L.check(self.lib.ov2_btracker_last_pose_inputs(self.h_trk, int(item), C.byref(m), slot.ctypes.data_as(C.POINTER(C.c_int)),
                                                       tab.ctypes.data_as(C.POINTER(C.c_int)), C.byref(rows)))
        return m.value, slot[:m.value].copy(), tab[:rows.value].copy()

    def setKeyframe(self, item, kf_lmid, kf_unpx, kf_bv, kf_Twc):
        """the keyframe item `item` is filtered against from now on (ov2_btracker_set_keyframe): kf_lmid (m,) strictly ascending,
        kf_unpx (m, 2), kf_bv (m, 3), kf_Twc (7,); it stays on the device until it is replaced.  m == 0 takes it away.  Between
        steps only."""
        lm = np.ascontiguousarray(kf_lmid, np.int32).reshape(-1)
        un = np.ascontiguousarray(kf_unpx, np.float32).reshape(-1, 2)
        bv = np.ascontiguousarray(kf_bv, np.float64).reshape(-1, 3)
        if len(un) != len(lm) or len(bv) != len(lm):
            raise ValueError("one unpx and one bearing per keyframe id")
        T = None if kf_Twc is None else np.ascontiguousarray(kf_Twc, np.float64).reshape(7)
        L.check(self.lib.ov2_btracker_set_keyframe(self.h_trk, int(item), len(lm), _ptr(lm), _ptr(un), _ptr(bv), _ptr(T)))

    def _epi_args(self, na, nn, params, epi_params, Twc, p3p_req, seed, lmid, nbkfs, epi_seed, scale, dop3p, n_rows):
        from . import keyframe as _kf
        fp, fi, keep = self._pose_args(na, nn, params, Twc, p3p_req, seed, scale, dop3p, n_rows)
        ep = L.FrameEpiPoseParams()
        ep.pose, ep.epi = fp, _kf._as_epifilter_params(epi_params)
        self._epi_rows = max(0, int(ep.epi.n_rows))                               # (the room lastEpiInputs gives the table)
        lm = np.ascontiguousarray(lmid, np.int32).reshape(self.batch, self.n_max)
        nk = np.ascontiguousarray(nbkfs, np.int32).reshape(-1)
        es = np.ascontiguousarray(epi_seed, np.uint64).reshape(-1)
        if len(nk) < na or len(es) < na:
            raise ValueError("one nbkfs and one epipolar seed per active item")
        ei = L.FrameEpiPoseInput()
        ei.pose = fi
        ei.lmid_h = lm.ctypes.data_as(C.POINTER(C.c_int))
        ei.nbkfs_h = nk.ctypes.data_as(C.POINTER(C.c_int))
        ei.epi_seed_h = es.ctypes.data_as(C.POINTER(C.c_ulonglong))
        return ep, ei, keep + (lm, nk, es)

    def _epi_results(self, na):
        R = (L.EpifilterResult * max(1, na))()
        bufs = dict(removed=np.zeros((max(1, na), self.n_max), np.uint8), pair_cur=np.zeros((max(1, na), self.n_max), np.int32),
                    err=np.zeros((max(1, na), self.n_max), np.float32))
        for b in range(na):
            R[b].removed = bufs["removed"][b].ctypes.data_as(C.POINTER(C.c_uint8))
            R[b].pair_cur = bufs["pair_cur"][b].ctypes.data_as(C.POINTER(C.c_int))
            R[b].err = bufs["err"][b].ctypes.data_as(C.POINTER(C.c_float))
        return R, bufs

    def _epi_dicts(self, R, bufs, nn):
        from . import keyframe as _kf
        return [_kf._epifilter_dict(R[b], dict(removed=bufs["removed"][b, :int(nn[b])], pair_cur=bufs["pair_cur"][b],
                                               err=bufs["err"][b, :int(nn[b])])) for b in range(len(nn))]

    def trackFrameEpiPose(self, imgs, kps, wpt, is3d, Tcw, n, params, epi_params, Twc, p3p_req, seed, lmid, nbkfs, epi_seed,
                          scale=None, dop3p=False, n_rows=0, klt_use_prior=True):
        """trackFrameMap, epipolar2d2dFiltering against the resident keyframes (setKeyframe) and the per-frame pose in one enqueue and
        one synchronisation (ov2_btracker_track_frame_epi_pose): trackMono's per-frame sequence with doepipolar_ == 1.  As
        trackFramePose, plus epi_params (as keyframe.epipolar_filter takes them; boptimize False), lmid (batch, n_max) int32, nbkfs
        and epi_seed one per item.  -> (out, status bits, p3p_req, epis, poses): epis[b] as keyframe.epipolar_filter returns it with
        removed / err (n[b],) and pair_cur (m,) IN SLOT SPACE; poses[b] as trackFramePose, on the frame after the filter."""
        na, imgs, stride, ptrs, kps, wpt, is3d, Tcw, nn = self._map_args(imgs, kps, wpt, is3d, Tcw, n)
        ep, ei, keep = self._epi_args(na, nn, params, epi_params, Twc, p3p_req, seed, lmid, nbkfs, epi_seed, scale, dop3p, n_rows)
        out, st, p3p = self._outputs(na)
        R, removed = self._pose_results(na, nn)
        E, bufs = self._epi_results(na)
        L.check(self.lib.ov2_btracker_track_frame_epi_pose(self.h_trk, na, ptrs, stride, _ptr(kps), _ptr(wpt), _ptr(is3d), _ptr(Tcw),
                                                           _ptr(nn), int(bool(klt_use_prior)), C.byref(ep), C.byref(ei), _ptr(out),
                                                           _ptr(st), _ptr(p3p), E, R))
        return out, st, p3p.astype(bool), self._epi_dicts(E, bufs, nn), self._pose_dicts(R, removed, nn)

    def trackFrameEpiPoseBegin(self, imgs, kps, wpt, is3d, Tcw, n, params, epi_params, Twc, p3p_req, seed, lmid, nbkfs, epi_seed,
                               scale=None, dop3p=False, n_rows=0, klt_use_prior=True):
        """first half of trackFrameEpiPose; trackFrameEpiPoseEnd finishes it (trackFrameEnd finishes the tracking half and drops both
        results)"""
        na, imgs, stride, ptrs, kps, wpt, is3d, Tcw, nn = self._map_args(imgs, kps, wpt, is3d, Tcw, n)
        ep, ei, keep = self._epi_args(na, nn, params, epi_params, Twc, p3p_req, seed, lmid, nbkfs, epi_seed, scale, dop3p, n_rows)
        L.check(self.lib.ov2_btracker_track_frame_epi_pose_begin(self.h_trk, na, ptrs, stride, _ptr(kps), _ptr(wpt), _ptr(is3d), _ptr(Tcw),
                                                                 _ptr(nn), int(bool(klt_use_prior)), C.byref(ep), C.byref(ei)))
        self._pending = (imgs, kps, wpt, is3d, nn)                                # (kps is re-read by the end half: keep it alive)

    def trackFrameEpiPoseEnd(self):
        """second half of trackFrameEpiPose -> (out, status bits, p3p_req, epis, poses)"""
        nn = self._pending[4]
        na = len(nn)
        out, st, p3p = self._outputs(na)
        R, removed = self._pose_results(na, nn)
        E, bufs = self._epi_results(na)
        L.check(self.lib.ov2_btracker_track_frame_epi_pose_end(self.h_trk, _ptr(out), _ptr(st), _ptr(p3p), E, R))
        self._pending = None
        return out, st, p3p.astype(bool), self._epi_dicts(E, bufs, nn), self._pose_dicts(R, removed, nn)

    def lastEpiInputs(self, item):
        """what the last epipolar step fed the filter for `item` -> (n_cur, slots (n_cur,) int32, m, samples (rows used, 8) int32)"""
        nc, m, rows = C.c_int(), C.c_int(), C.c_int()
        slot = np.zeros(self.n_max, np.int32)
        tab = np.zeros((max(1, self._epi_rows), 8), np.int32)
        L.check(self.lib.ov2_btracker_last_epi_inputs(self.h_trk, int(item), C.byref(nc), slot.ctypes.data_as(C.POINTER(C.c_int)),
                                                      C.byref(m), tab.ctypes.data_as(C.POINTER(C.c_int)), C.byref(rows)))
        return nc.value, slot[:nc.value].copy(), m.value, tab[:rows.value].copy()

    # ---- trackMono after initialisation in one step (ov2_btracker_track_mono) --------------------------------------------------
    def setPose(self, item, Twc):
        """the frame pose of item `item` (pcurframe_->Twc_), resident on the device: the estimator or the loop closer moved the frame.
        Between steps only."""
        T = np.ascontiguousarray(Twc, np.float64).reshape(7)
        L.check(self.lib.ov2_btracker_set_pose(self.h_trk, int(item), _ptr(T)))

    def getPose(self, item):
        T = np.zeros(7)
        L.check(self.lib.ov2_btracker_get_pose(self.h_trk, int(item), _ptr(T)))
        return T

    def resetMotion(self, item):
        """MotionModel::reset() of item `item`"""
        L.check(self.lib.ov2_btracker_reset_motion(self.h_trk, int(item)))

    def getMotion(self, item):
        """the motion state of item `item` as motion.apply takes it"""
        from . import motion as _motion
        s = L.MotionState()
        L.check(self.lib.ov2_btracker_get_motion(self.h_trk, int(item), C.byref(s)))
        return _motion._state_dict(s)

    def setKeyframeInfo(self, item, kf_id, kf_time, kf_nb3dkps):
        """id_, img_time_ and nb3dkps_ of the keyframe setKeyframe gave item `item`"""
        L.check(self.lib.ov2_btracker_set_keyframe_info(self.h_trk, int(item), int(kf_id), float(kf_time), int(kf_nb3dkps)))

    def _mono_args(self, na, nn, params, epi_params, p3p_req, seed, lmid, nbkfs, epi_seed, time, frame_id, localba_is_on, doepipolar,
                   scale, dop3p, n_rows):
        ep, ei, keep = self._epi_args(na, nn, params, epi_params, np.zeros((max(1, na), 7)), p3p_req, seed,
                                      np.zeros((self.batch, self.n_max), np.int32) if lmid is None else lmid,
                                      np.zeros(self.batch, np.int32) if nbkfs is None else nbkfs,
                                      np.zeros(self.batch, np.uint64) if epi_seed is None else epi_seed, scale, dop3p, n_rows)
        ei.pose.Twc_h = None                                                      # the pose is resident
        if lmid is None:
            ei.lmid_h = None                                                      # ... and so is the frame (trackMonoResident)
        mp, mi = L.TrackMonoParams(), L.TrackMonoInput()
        mp.step, mp.doepipolar = ep, int(bool(doepipolar))
        tm = np.ascontiguousarray(time, np.float64).reshape(-1)
        fid = np.ascontiguousarray(frame_id, np.int32).reshape(-1)
        ba = None if localba_is_on is None else np.ascontiguousarray(localba_is_on, np.uint8).reshape(-1)
        if len(tm) < na or len(fid) < na or (ba is not None and len(ba) < na):
            raise ValueError("one time, one frame id and one local-BA flag per active item")
        mi.step = ei
        mi.time_h = tm.ctypes.data_as(C.POINTER(C.c_double))
        mi.frame_id_h = fid.ctypes.data_as(C.POINTER(C.c_int))
        mi.localba_is_on_h = None if ba is None else ba.ctypes.data_as(C.POINTER(C.c_uint8))
        self._mono_epi = bool(doepipolar)
        return mp, mi, keep + (tm, fid, ba)

    def _mono_dicts(self, M, na):
        from . import keyframe as _kf
        from . import motion as _motion
        return [dict(Twc_pred=np.array(M[b].Twc_pred[:], np.float64), resynced=int(M[b].resynced), state=_motion._state_dict(M[b].state),
                     kf=_kf._decision_dict(M[b].kf)) for b in range(na)]

    def _map_args_mono(self, imgs, kps, wpt, is3d, n):
        return self._map_args(imgs, kps, wpt, is3d, np.zeros((max(1, len(imgs)), 7)), n)

    def trackMono(self, imgs, kps, wpt, is3d, n, params, epi_params, p3p_req, seed, lmid, nbkfs, epi_seed, time, frame_id,
                  localba_is_on=None, doepipolar=True, scale=None, dop3p=False, n_rows=0, klt_use_prior=True):
        """VisualFrontEnd::trackMono after initialisation in one enqueue and one synchronisation (ov2_btracker_track_mono): the motion
        model on the resident pose (setPose / getPose) and state (resetMotion / getMotion), trackFrameEpiPose (doepipolar False:
        trackFramePose) from the predicted pose, updateMotionModel and checkNewKfReq against the resident keyframe (setKeyframe,
        setKeyframeInfo).  As trackFrameEpiPose without Tcw and Twc, plus time, frame_id and localba_is_on one per item.
        -> (out, status bits, p3p_req, epis (None with doepipolar False), poses, monos): monos[b] = dict(Twc_pred (7,), resynced,
        state (the motion state after the update), kf (as keyframe.kf_decision returns it))."""
        na, imgs, stride, ptrs, kps, wpt, is3d, _, nn = self._map_args_mono(imgs, kps, wpt, is3d, n)
        mp, mi, keep = self._mono_args(na, nn, params, epi_params, p3p_req, seed, lmid, nbkfs, epi_seed, time, frame_id, localba_is_on,
                                       doepipolar, scale, dop3p, n_rows)
        out, st, p3p = self._outputs(na)
        R, removed = self._pose_results(na, nn)
        E, bufs = self._epi_results(na)
        M = (L.TrackMonoResult * max(1, na))()
        L.check(self.lib.ov2_btracker_track_mono(self.h_trk, na, ptrs, stride, _ptr(kps), _ptr(wpt), _ptr(is3d), _ptr(nn),
                                                 int(bool(klt_use_prior)), C.byref(mp), C.byref(mi), _ptr(out), _ptr(st), _ptr(p3p),
                                                 E if doepipolar else None, R, M))
        return (out, st, p3p.astype(bool), self._epi_dicts(E, bufs, nn) if doepipolar else None, self._pose_dicts(R, removed, nn),
                self._mono_dicts(M, na))

    def trackMonoBegin(self, imgs, kps, wpt, is3d, n, params, epi_params, p3p_req, seed, lmid, nbkfs, epi_seed, time, frame_id,
                       localba_is_on=None, doepipolar=True, scale=None, dop3p=False, n_rows=0, klt_use_prior=True):
        """first half of trackMono; trackMonoEnd finishes it (trackFrameEnd gives the tracking half, drops the rest and leaves the
        resident pose and state as they were)"""
        na, imgs, stride, ptrs, kps, wpt, is3d, _, nn = self._map_args_mono(imgs, kps, wpt, is3d, n)
        mp, mi, keep = self._mono_args(na, nn, params, epi_params, p3p_req, seed, lmid, nbkfs, epi_seed, time, frame_id, localba_is_on,
                                       doepipolar, scale, dop3p, n_rows)
        L.check(self.lib.ov2_btracker_track_mono_begin(self.h_trk, na, ptrs, stride, _ptr(kps), _ptr(wpt), _ptr(is3d), _ptr(nn),
                                                       int(bool(klt_use_prior)), C.byref(mp), C.byref(mi)))
        self._pending = (imgs, kps, wpt, is3d, nn)                                # (kps is re-read by the end half: keep it alive)

    def trackMonoEnd(self):
        """second half of trackMono -> (out, status bits, p3p_req, epis, poses, monos)"""
        nn = self._pending[4]
        na = len(nn)
        out, st, p3p = self._outputs(na)
        R, removed = self._pose_results(na, nn)
        E, bufs = self._epi_results(na)
        M = (L.TrackMonoResult * max(1, na))()
        L.check(self.lib.ov2_btracker_track_mono_end(self.h_trk, _ptr(out), _ptr(st), _ptr(p3p), E if self._mono_epi else None, R, M))
        self._pending = None
        return (out, st, p3p.astype(bool), self._epi_dicts(E, bufs, nn) if self._mono_epi else None, self._pose_dicts(R, removed, nn),
                self._mono_dicts(M, na))

    # ---- the current frame resident on the device between the steps (ov2_btracker_set_frame, ..._track_mono_resident) -------------
    def setFrame(self, item, px, lmid, is3d, wpt):
        """installs the current frame of item `item` on the device (ov2_btracker_set_frame): px (n, 2), lmid (n,) distinct and >= 0,
        is3d (n,), wpt (n, 3), n <= n_max.  The first install, and the fallback where createKeyframe did not create.  Between
        steps only."""
        px = np.ascontiguousarray(px, np.float32).reshape(-1, 2)
        lm = np.ascontiguousarray(lmid, np.int32).reshape(-1)
        d3 = np.ascontiguousarray(is3d, np.uint8).reshape(-1)
        w = np.ascontiguousarray(wpt, np.float64).reshape(-1, 3)
        if not (len(px) == len(lm) == len(d3) == len(w)):
            raise ValueError("one px, one lmid, one is3d and one wpt per slot")
        L.check(self.lib.ov2_btracker_set_frame(self.h_trk, int(item), len(lm), _ptr(px), _ptr(lm), _ptr(d3), _ptr(w)))

    def getFrame(self, item, from_device=True):
        """the resident frame of item `item` -> dict(n, px (n, 2), lmid (n,), is3d (n,), wpt (n, 3)): copied down from the device
        block, or with from_device False the host mirror.  wpt of a slot that is not 3-D is whatever the slot last carried."""
        n = C.c_int()
        px, lm = np.zeros((self.n_max, 2), np.float32), np.zeros(self.n_max, np.int32)
        d3, w = np.zeros(self.n_max, np.uint8), np.zeros((self.n_max, 3), np.float64)
        L.check(self.lib.ov2_btracker_get_frame(self.h_trk, int(item), int(bool(from_device)), C.byref(n), _ptr(px), _ptr(lm), _ptr(d3), _ptr(w)))
        k = n.value
        return dict(n=k, px=px[:k].copy(), lmid=lm[:k].copy(), is3d=d3[:k].copy(), wpt=w[:k].copy())

    def updateFrame(self, n_active, ops):
        """what the map did to the resident frames of items [0, n_active) since the last step (ov2_btracker_update_frame_batch), one
        upload, one launch, one download: ops[b] is a list of (lmid, op, xyz) with op L.OV2_RES_SET_POINT (wpt = xyz, is3d = 1),
        L.OV2_RES_UNSET_POINT (is3d = 0) or L.OV2_RES_REMOVE (the slot leaves, the rest close up in slot order); xyz may be None
        where the op does not read it.  An lmid the frame does not hold is counted.
        -> [dict(n_before, n_after, n_set, n_unset, n_removed, n_missing)] per item"""
        na = int(n_active)
        if len(ops) < na:
            raise ValueError("one op list per active item")
        lists, cnt = [], np.zeros(max(1, na), np.int32)
        ptrs = (C.POINTER(L.ResidentOp) * max(1, na))()
        for b in range(na):
            arr = (L.ResidentOp * max(1, len(ops[b])))()
            for j, (lmid, op, xyz) in enumerate(ops[b]):
                arr[j].lmid, arr[j].op = int(lmid), int(op)
                arr[j].xyz = (C.c_double * 3)(*([0.0, 0.0, 0.0] if xyz is None else [float(v) for v in xyz]))
            lists.append(arr)
            cnt[b] = len(ops[b])
            ptrs[b] = C.cast(arr, C.POINTER(L.ResidentOp))
        R = (L.ResidentUpdateResult * max(1, na))()
        L.check(self.lib.ov2_btracker_update_frame_batch(self.h_trk, na, cnt.ctypes.data_as(C.POINTER(C.c_int)), ptrs, R))
        return [{k: int(getattr(R[b], k)) for k, _ in L.ResidentUpdateResult._fields_} for b in range(na)]

    def lastSlotBytes(self):
        """bytes of per-slot input (keypoints, points, flags, ids, scales: anything sized by n or n_max; not images) the last step or
        createKeyframe call wrote for the device: 0 for the resident forms"""
        v = C.c_size_t()
        L.check(self.lib.ov2_btracker_last_slot_bytes(self.h_trk, C.byref(v)))
        return int(v.value)

    def _resident_args(self, imgs, params, epi_params, p3p_req, seed, nbkfs, epi_seed, time, frame_id, localba_is_on, doepipolar, dop3p,
                       n_rows):
        na = len(imgs)
        imgs, stride, ptrs = self._frames(imgs)
        mp, mi, keep = self._mono_args(na, None, params, epi_params, p3p_req, seed, None, nbkfs, epi_seed, time, frame_id, localba_is_on,
                                       doepipolar, None, dop3p, n_rows)
        return na, imgs, stride, ptrs, mp, mi, keep

    def _resident_results(self, na):
        out, st, p3p = self._outputs(na)
        R, removed = self._pose_results(na, None)
        E, bufs = self._epi_results(na)
        return out, st, p3p, R, removed, E, bufs, (L.TrackMonoResult * max(1, na))(), (L.ResidentStepResult * max(1, na))()

    def _resident_return(self, na, out, st, p3p, R, removed, E, bufs, M, F, epi):
        nn = np.array([F[b].n_before for b in range(na)], np.int32)
        return (out, st, p3p.astype(bool), self._epi_dicts(E, bufs, nn) if epi else None, self._pose_dicts(R, removed, nn),
                self._mono_dicts(M, na), [dict(n_before=int(F[b].n_before), n_after=int(F[b].n_after)) for b in range(na)])

    def trackMonoResident(self, imgs, params, epi_params, p3p_req, seed, nbkfs, epi_seed, time, frame_id, localba_is_on=None,
                          doepipolar=True, dop3p=False, n_rows=0, klt_use_prior=True):
        """trackMono on the resident frames (ov2_btracker_track_mono_resident): as trackMono without kps, wpt, is3d, n, lmid and scale
        -- the frame of each item is the one setFrame / updateFrame / createKeyframe / the last step left on the device, and the
        step leaves its successor there: the tracked px of the slots that are tracked and were removed by neither the filter nor the
        pose, with their lmid, is3d and wpt, in slot order.
        -> (out, status bits, p3p_req, epis, poses, monos, frames): as trackMono, in the slot space of the frame BEFORE the step;
        frames[b] = dict(n_before, n_after)."""
        na, imgs, stride, ptrs, mp, mi, keep = self._resident_args(imgs, params, epi_params, p3p_req, seed, nbkfs, epi_seed, time, frame_id,
                                                                   localba_is_on, doepipolar, dop3p, n_rows)
        out, st, p3p, R, removed, E, bufs, M, F = self._resident_results(na)
        L.check(self.lib.ov2_btracker_track_mono_resident(self.h_trk, na, ptrs, stride, int(bool(klt_use_prior)), C.byref(mp), C.byref(mi),
                                                          _ptr(out), _ptr(st), _ptr(p3p), E if doepipolar else None, R, M, F))
        return self._resident_return(na, out, st, p3p, R, removed, E, bufs, M, F, doepipolar)

    def trackMonoResidentBegin(self, imgs, params, epi_params, p3p_req, seed, nbkfs, epi_seed, time, frame_id, localba_is_on=None,
                               doepipolar=True, dop3p=False, n_rows=0, klt_use_prior=True):
        """first half of trackMonoResident; trackMonoResidentEnd finishes it (trackFrameEnd gives the tracking half, drops the rest and
        leaves the resident pose, state and frames as they were)"""
        na, imgs, stride, ptrs, mp, mi, keep = self._resident_args(imgs, params, epi_params, p3p_req, seed, nbkfs, epi_seed, time, frame_id,
                                                                   localba_is_on, doepipolar, dop3p, n_rows)
        L.check(self.lib.ov2_btracker_track_mono_resident_begin(self.h_trk, na, ptrs, stride, int(bool(klt_use_prior)), C.byref(mp), C.byref(mi)))
        self._pending = (imgs, None, None, None, np.zeros(na, np.int32))

    def trackMonoResidentEnd(self):
        """second half of trackMonoResident -> (out, status bits, p3p_req, epis, poses, monos, frames)"""
        na = len(self._pending[4])
        out, st, p3p, R, removed, E, bufs, M, F = self._resident_results(na)
        L.check(self.lib.ov2_btracker_track_mono_resident_end(self.h_trk, _ptr(out), _ptr(st), _ptr(p3p), E if self._mono_epi else None, R, M, F))
        self._pending = None
        return self._resident_return(na, out, st, p3p, R, removed, E, bufs, M, F, self._mono_epi)

    # ---- createKeyframe for the items a step flagged (ov2_btracker_create_keyframe) ------------------------------------------------
    def _ckf_args(self, n_active, px, lmid, is3d, n, make_kf, nlmid, nkfid, time, params, state, Twc):
        na = int(n_active)
        cp = L.CreateKeyframeParams()
        cp.ncellsize, cp.nbwcells, cp.nbhcells, cp.nbmaxkps = (int(params[k]) for k in ("ncellsize", "nbwcells", "nbhcells", "nbmaxkps"))
        det = params.get("detector", "singlescale")
        cp.detector = {"singlescale": L.OV2_CKF_DET_SINGLESCALE, "gridfast": L.OV2_CKF_DET_GRID_FAST, "gftt": L.OV2_CKF_DET_GFTT}.get(det, det)
        cp.det_cell = int(params["det_cell"])
        cp.roi = (C.c_int * 4)(*[int(v) for v in params.get("roi", (0, 0, self.w, self.h))])
        cp.mask_mode = int(params.get("mask_mode", L.OV2_MASK_AS_EXECUTED))
        cp.do_subpix, cp.use_brief = int(bool(params.get("do_subpix", True))), int(bool(params.get("use_brief", True)))
        resident = px is None                                                     # the frame is the resident one
        if resident and not (lmid is None and is3d is None and n is None):
            raise ValueError("px None means the resident frame: lmid, is3d and n must be None too")
        px = None if resident else np.ascontiguousarray(px, np.float32).reshape(self.batch, self.n_max, 2)
        lm = None if resident else np.ascontiguousarray(lmid, np.int32).reshape(self.batch, self.n_max)
        d3 = None if resident else np.ascontiguousarray(is3d, np.uint8).reshape(self.batch, self.n_max)
        nn = np.zeros(na, np.int32) if resident else np.ascontiguousarray(n, np.int32).reshape(-1)
        mk = np.ascontiguousarray(make_kf, np.uint8).reshape(-1)
        nl = np.ascontiguousarray(nlmid, np.int32).reshape(-1)
        ki = np.ascontiguousarray(nkfid, np.int32).reshape(-1)
        tm = np.ascontiguousarray(time, np.float64).reshape(-1)
        if min(len(nn), len(mk), len(nl), len(ki), len(tm)) < na:
            raise ValueError("one count, flag, nlmid, keyframe id and time per active item")
        T = None if Twc is None else np.ascontiguousarray(Twc, np.float64).reshape(-1, 7)
        if T is not None and len(T) < na:
            raise ValueError("one pose per active item")
        fast = cp.detector == L.OV2_CKF_DET_GRID_FAST
        st = np.ascontiguousarray(state, np.int32 if fast else np.float64)
        assert st is state or np.shares_memory(st, state), "state must be a contiguous int32 (FAST) / float64 (single scale) array (updated in place)"
        if len(st) < na:
            raise ValueError("one adaptive state per active item")
        ci = L.CreateKeyframeInput()
        ci.px_h = None if resident else px.ctypes.data_as(C.POINTER(C.c_float))
        ci.lmid_h = None if resident else lm.ctypes.data_as(C.POINTER(C.c_int))
        ci.is3d_h = None if resident else d3.ctypes.data_as(C.POINTER(C.c_uint8))
        ci.n_h = None if resident else nn.ctypes.data_as(C.POINTER(C.c_int))
        ci.make_kf_h = mk.ctypes.data_as(C.POINTER(C.c_uint8))
        ci.nlmid_h = nl.ctypes.data_as(C.POINTER(C.c_int))
        ci.nkfid_h = ki.ctypes.data_as(C.POINTER(C.c_int))
        ci.time_h = tm.ctypes.data_as(C.POINTER(C.c_double))
        ci.Twc_h = None if T is None else T.ctypes.data_as(C.POINTER(C.c_double))
        ci.quality_inout = None if fast else st.ctypes.data_as(C.POINTER(C.c_double))
        ci.fast_th_inout = st.ctypes.data_as(C.POINTER(C.c_int)) if fast else None
        return na, cp, ci, (px, lm, d3, nn, mk, nl, ki, tm, T, st)

    def _ckf_outputs(self, na, out):
        """the arrays _end scatters into (the caller's, so that untouched slots stay what they were, or fresh zeros)"""
        shapes = dict(px=((self.batch, self.n_max, 2), np.float32), lmid=((self.batch, self.n_max), np.int32),
                      unpx=((self.batch, self.n_max, 2), np.float32), bv=((self.batch, self.n_max, 3), np.float64),
                      desc=((self.batch, self.n_max, L.OV2_BRIEF_BYTES), np.uint8), valid=((self.batch, self.n_max), np.uint8),
                      color=((self.batch, self.n_max), np.uint8))
        o = {}
        for k, (shape, dt) in shapes.items():
            a = None if out is None else out.get(k)
            if a is None:
                a = np.zeros(shape, dt)
            elif a.dtype != dt or a.shape != shape or not a.flags.c_contiguous:
                raise ValueError("out[%r] must be a contiguous %s array of shape %r" % (k, np.dtype(dt).name, shape))
            o[k] = a
        return o, (L.CreateKeyframeResult * max(1, na))()

    def _ckf_dicts(self, R, na, o):
        keys = ("action", "n_prev", "noccupcells", "nb2detect", "n_new", "n_kf", "nb3dkps")
        return [{k: int(getattr(R[b], k)) for k in keys} for b in range(na)], o

    def createKeyframe(self, n_active, px, lmid, is3d, n, make_kf, nlmid, nkfid, time, params, state, Twc=None, out=None):
        """MapManager::createKeyframe for the items of [0, n_active) with make_kf[b] != 0, in one enqueue and one synchronisation
        (ov2_btracker_create_keyframe): describeBRIEF, the detector's top-up of the empty cells, addKeypointsToFrame, computeKeypoint and
        the new frame installed as the item's resident keyframe (setKeyframe + setKeyframeInfo) without leaving the device.
        px (batch, n_max, 2), lmid / is3d (batch, n_max), n: the current frame after prepareFrame; nlmid, nkfid, time: one per item;
        params: dict(ncellsize, nbwcells, nbhcells, nbmaxkps, detector "singlescale" | "gridfast", det_cell, roi, mask_mode, do_subpix,
        use_brief); state: float64 qualities (single scale) or int32 thresholds (FAST), one per item, updated in place; Twc
        (>= n_active, 7) or None: the resident pose; out: dict of arrays to scatter into (missing ones are zeros).
        px None (with lmid, is3d and n None): the frames are the resident ones (setFrame, trackMonoResident); nothing per slot
        goes up, and the frame with the new points appended (is3d 0, wpt 0) becomes the resident frame of every CREATED item.
        -> (records, out): records[b] = dict(action, n_prev, noccupcells, nb2detect, n_new, n_kf, nb3dkps); out = dict(px, lmid, unpx,
        bv, desc, valid, color) in slot layout, written for the items with action OV2_CKF_CREATED only."""
        na, cp, ci, keep = self._ckf_args(n_active, px, lmid, is3d, n, make_kf, nlmid, nkfid, time, params, state, Twc)
        o, R = self._ckf_outputs(na, out)
        L.check(self.lib.ov2_btracker_create_keyframe(self.h_trk, na, C.byref(cp), C.byref(ci), R, _ptr(o["px"]), _ptr(o["lmid"]), _ptr(o["unpx"]),
                                                      _ptr(o["bv"]), _ptr(o["desc"]), _ptr(o["valid"]), _ptr(o["color"])))
        return self._ckf_dicts(R, na, o)

    def createKeyframeBegin(self, n_active, px, lmid, is3d, n, make_kf, nlmid, nkfid, time, params, state, Twc=None):
        """first half of createKeyframe: enqueue and return; createKeyframeEnd finishes it (state is updated there: keep it alive)"""
        na, cp, ci, keep = self._ckf_args(n_active, px, lmid, is3d, n, make_kf, nlmid, nkfid, time, params, state, Twc)
        L.check(self.lib.ov2_btracker_create_keyframe_begin(self.h_trk, na, C.byref(cp), C.byref(ci)))
        self._ckf_pending = (na, keep)

    def createKeyframeEnd(self, out=None):
        """second half of createKeyframe -> (records, out)"""
        na = self._ckf_pending[0] if getattr(self, "_ckf_pending", None) else 0          # (no open call: the library refuses)
        o, R = self._ckf_outputs(na, out)
        L.check(self.lib.ov2_btracker_create_keyframe_end(self.h_trk, R, _ptr(o["px"]), _ptr(o["lmid"]), _ptr(o["unpx"]), _ptr(o["bv"]),
                                                          _ptr(o["desc"]), _ptr(o["valid"]), _ptr(o["color"])))
        self._ckf_pending = None
        return self._ckf_dicts(R, na, o)

    # ---- the mapper's stereo block on the resident keyframe (ov2_btracker_stereo_keyframe) -----------------------------------------
    def _skf_outputs(self, na, out):
        """the arrays _end scatters into (the caller's, so that untouched slots stay what they were, or fresh zeros)"""
        shapes = dict(right_px=((self.batch, self.n_max, 2), np.float32), stereo_ok=((self.batch, self.n_max), np.uint8),
                      tri_status=((self.batch, self.n_max), np.uint8), wpt=((self.batch, self.n_max, 3), np.float64),
                      invdepth=((self.batch, self.n_max), np.float64))
        o = {}
        for k, (shape, dt) in shapes.items():
            a = None if out is None else out.get(k)
            if a is None:
                a = np.zeros(shape, dt)
            elif a.dtype != dt or a.shape != shape or not a.flags.c_contiguous:
                raise ValueError("out[%r] must be a contiguous %s array of shape %r" % (k, np.dtype(dt).name, shape))
            o[k] = a
        return o, (L.StereoKeyframeResult * max(1, na))()

    def _skf_dicts(self, R, na, o):
        return [{k: int(getattr(R[b], k)) for k, _ in L.StereoKeyframeResult._fields_} for b in range(na)], o

    @staticmethod
    def _skf_do(n_active, do):
        na = int(n_active)
        d = np.ascontiguousarray(do, np.uint8).reshape(-1)
        if len(d) < na:
            raise ValueError("one flag per active item")
        return na, d

    def stereoKeyframe(self, n_active, right_pyr, do, params, out=None):
        """MapManager::stereoMatching, then Mapper::triangulateStereo, on the resident keyframe of the items of [0, n_active) with
        do[b] != 0 (normally: the item's last createKeyframe action was OV2_CKF_CREATED), in one enqueue and one synchronisation
        (ov2_btracker_stereo_keyframe): the stereo priors, the line search (rect), the tracking from cur_pyr into right_pyr, the
        epipolar gate, the right camera's computeKeypoint, triangulateStereo; every OV2_TRI_STEREO_OK slot becomes 3-D in the
        resident frame and the keyframe info's kf_nb3dkps is recounted.  right_pyr: a batch Pyramid of the right images on this
        tracker's context (it may still be building); params: mapper.stereo_keyframe_params(...); out: dict of arrays to scatter
        into (missing ones are zeros).  Keypoints of a grid cell stand in slot order (not vgridkps_ insertion order); state 2
        cannot occur (remove such observations with updateFrame first); triangulateTemporal is not run.
        -> (records, out): records[b] = dict(action L.OV2_SKF_*, n, n_prior3d, n_prior_nb, n_stereo_kps, n_stereo, n_stereo_good,
        nb3dkps); out = dict(right_px, stereo_ok, tri_status, wpt, invdepth) in the slot layout of the resident frame, written
        for the items with action OV2_SKF_DONE only."""
        na, d = self._skf_do(n_active, do)
        o, R = self._skf_outputs(na, out)
        L.check(self.lib.ov2_btracker_stereo_keyframe(self.h_trk, na, C.byref(params), right_pyr.h_pyr, _ptr(d), R, _ptr(o["right_px"]),
                                                      _ptr(o["stereo_ok"]), _ptr(o["tri_status"]), _ptr(o["wpt"]), _ptr(o["invdepth"])))
        return self._skf_dicts(R, na, o)

    def stereoKeyframeBegin(self, n_active, right_pyr, do, params):
        """first half of stereoKeyframe: enqueue and return; stereoKeyframeEnd finishes it"""
        na, d = self._skf_do(n_active, do)
        L.check(self.lib.ov2_btracker_stereo_keyframe_begin(self.h_trk, na, C.byref(params), right_pyr.h_pyr, _ptr(d)))
        self._skf_pending = (na, right_pyr, params)

    def stereoKeyframeEnd(self, out=None):
        """second half of stereoKeyframe -> (records, out)"""
        na = self._skf_pending[0] if getattr(self, "_skf_pending", None) else 0          # (no open call: the library refuses)
        o, R = self._skf_outputs(na, out)
        L.check(self.lib.ov2_btracker_stereo_keyframe_end(self.h_trk, R, _ptr(o["right_px"]), _ptr(o["stereo_ok"]), _ptr(o["tri_status"]),
                                                          _ptr(o["wpt"]), _ptr(o["invdepth"])))
        self._skf_pending = None
        return self._skf_dicts(R, na, o)

    def getKeyframeInfo(self, item, from_device=False):
        """the resident keyframe info of item `item` -> dict(kf_id, kf_time, kf_nb3dkps, has_info): the host mirror, or with
        from_device True copied down from the device block"""
        i, t, n, hi = C.c_int(), C.c_double(), C.c_int(), C.c_int()
        L.check(self.lib.ov2_btracker_get_keyframe_info(self.h_trk, int(item), int(bool(from_device)), C.byref(i), C.byref(t), C.byref(n),
                                                        C.byref(hi)))
        return dict(kf_id=i.value, kf_time=t.value, kf_nb3dkps=n.value, has_info=hi.value)

    # ---- Mapper::triangulateTemporal on the resident keyframe (ov2_btracker_temporal_keyframe) and the anchor table -----------------
    def reserveAnchors(self, n_src_max):
        """allocates the anchor block with n_src_max rows per item (ov2_btracker_reserve_anchors); the first temporalKeyframe does
        it otherwise.  Another n_src_max afterwards is refused."""
        L.check(self.lib.ov2_btracker_reserve_anchors(self.h_trk, int(n_src_max)))
        self._n_src_max = int(n_src_max)

    def setAnchors(self, item, lmid, kfid, unpx, bv, row_kfid, row_Twc):
        """installs the whole anchor table of item `item` (ov2_btracker_set_anchors), as setKeyframe installs a keyframe: per keypoint
        of the latest keyframe lmid (n,) strictly ascending, kfid (n,) its first observing keyframe, unpx (n, 2) and bv (n, 3) its
        keypoint there; per keyframe referred to row_kfid (r,) strictly ascending and row_Twc (r, 7).  After the map culled a
        keyframe, or for a tracker that joins a running map.  Between steps only."""
        lm = np.ascontiguousarray(lmid, np.int32).reshape(-1)
        kf = np.ascontiguousarray(kfid, np.int32).reshape(-1)
        un = np.ascontiguousarray(unpx, np.float32).reshape(-1, 2)
        b = np.ascontiguousarray(bv, np.float64).reshape(-1, 3)
        rk = np.ascontiguousarray(row_kfid, np.int32).reshape(-1)
        rT = np.ascontiguousarray(row_Twc, np.float64).reshape(-1, 7)
        if not (len(lm) == len(kf) == len(un) == len(b)) or len(rk) != len(rT):
            raise ValueError("one kfid, unpx and bv per lmid, one pose per row")
        L.check(self.lib.ov2_btracker_set_anchors(self.h_trk, int(item), len(lm), _ptr(lm), _ptr(kf), _ptr(un), _ptr(b), len(rk), _ptr(rk), _ptr(rT)))

    def getAnchors(self, item, from_device=False):
        """the anchor table of item `item` -> dict(n, lmid (n,), kfid (n,), unpx (n, 2), bv (n, 3), n_rows, row_kfid (r,), row_Twc (r, 7),
        row_Tcw (r, 7)): the host mirror, or with from_device True copied down from the device block"""
        ns = getattr(self, "_n_src_max", L.OV2_TKF_MAX_ROWS)
        n, nr = C.c_int(), C.c_int()
        lm, kf = np.zeros(self.n_max, np.int32), np.zeros(self.n_max, np.int32)
        un, b = np.zeros((self.n_max, 2), np.float32), np.zeros((self.n_max, 3), np.float64)
        rk, rT, rI = np.zeros(ns, np.int32), np.zeros((ns, 7), np.float64), np.zeros((ns, 7), np.float64)
        L.check(self.lib.ov2_btracker_get_anchors(self.h_trk, int(item), int(bool(from_device)), C.byref(n), _ptr(lm), _ptr(kf), _ptr(un), _ptr(b),
                                                  C.byref(nr), _ptr(rk), _ptr(rT), _ptr(rI)))
        k, r = n.value, nr.value
        return dict(n=k, lmid=lm[:k].copy(), kfid=kf[:k].copy(), unpx=un[:k].copy(), bv=b[:k].copy(), n_rows=r, row_kfid=rk[:r].copy(),
                    row_Twc=rT[:r].copy(), row_Tcw=rI[:r].copy())

    def setAnchorPoses(self, triples):
        """the poses local BA moved (ov2_btracker_set_anchor_poses_batch): triples is a list of (item, kfid, Twc (7,)); one upload and
        one launch for all of them.  -> the number of triples whose kfid anchors nothing in its item (ignored)"""
        it = np.ascontiguousarray([t[0] for t in triples], np.int32).reshape(-1)
        kf = np.ascontiguousarray([t[1] for t in triples], np.int32).reshape(-1)
        T = np.ascontiguousarray([t[2] for t in triples], np.float64).reshape(-1, 7)
        ign = C.c_int()
        L.check(self.lib.ov2_btracker_set_anchor_poses_batch(self.h_trk, len(it), _ptr(it), _ptr(kf), _ptr(T), C.byref(ign)))
        return ign.value

    def _tkf_outputs(self, na, out):
        """the arrays _end scatters into (the caller's, so that untouched slots stay what they were, or fresh zeros)"""
        shapes = dict(tri_status=((self.batch, self.n_max), np.uint8), wpt=((self.batch, self.n_max, 3), np.float64),
                      invdepth=((self.batch, self.n_max), np.float64), src_kfid=((self.batch, self.n_max), np.int32))
        o = {}
        for k, (shape, dt) in shapes.items():
            a = None if out is None else out.get(k)
            if a is None:
                a = np.zeros(shape, dt)
            elif a.dtype != dt or a.shape != shape or not a.flags.c_contiguous:
                raise ValueError("out[%r] must be a contiguous %s array of shape %r" % (k, np.dtype(dt).name, shape))
            o[k] = a
        return o, (L.TemporalKeyframeResult * max(1, na))()

    def _tkf_dicts(self, R, na, o):
        return [{k: int(getattr(R[b], k)) for k, _ in L.TemporalKeyframeResult._fields_} for b in range(na)], o

    def temporalKeyframe(self, n_active, do, params, out=None):
        """Mapper::triangulateTemporal on the resident keyframe of the items of [0, n_active) with do[b] != 0 (normally: the item's
        last createKeyframe action was OV2_CKF_CREATED; in stereo behind stereoKeyframe), in one enqueue and one synchronisation
        (ov2_btracker_temporal_keyframe): the item's anchor table moves on to this keyframe, every 2-D slot the keyframe holds whose
        anchor is an earlier keyframe is triangulated against it, every OV2_TRI_TEMPORAL_OK slot becomes 3-D in the resident
        frame, every OV2_TRI_REMOVE_OBS slot leaves the resident keyframe, kf_nb3dkps is recounted.  params:
        mapper.temporal_keyframe_params(...); out: dict of arrays to scatter into (missing ones are zeros).  Points first seen at a
        keyframe for which this call was not run anchor at the next one for which it is.
        -> (records, out): records[b] = dict(action L.OV2_TKF_*, n, n_candidates, n_temporal_good, n_remove_obs, n_no_motion, nb3dkps,
        n_rows); out = dict(tri_status, wpt, invdepth, src_kfid) in the slot layout of the resident frame, written for the items with
        action OV2_TKF_DONE only."""
        na, d = self._skf_do(n_active, do)
        o, R = self._tkf_outputs(na, out)
        L.check(self.lib.ov2_btracker_temporal_keyframe(self.h_trk, na, C.byref(params), _ptr(d), R, _ptr(o["tri_status"]), _ptr(o["wpt"]),
                                                        _ptr(o["invdepth"]), _ptr(o["src_kfid"])))
        self._n_src_max = int(params.n_src_max)
        return self._tkf_dicts(R, na, o)

    def temporalKeyframeBegin(self, n_active, do, params):
        """first half of temporalKeyframe: enqueue and return; temporalKeyframeEnd finishes it"""
        na, d = self._skf_do(n_active, do)
        L.check(self.lib.ov2_btracker_temporal_keyframe_begin(self.h_trk, na, C.byref(params), _ptr(d)))
        self._n_src_max = int(params.n_src_max)
        self._tkf_pending = (na, params)

    def temporalKeyframeEnd(self, out=None):
        """second half of temporalKeyframe -> (records, out)"""
        na = self._tkf_pending[0] if getattr(self, "_tkf_pending", None) else 0          # (no open call: the library refuses)
        o, R = self._tkf_outputs(na, out)
        L.check(self.lib.ov2_btracker_temporal_keyframe_end(self.h_trk, R, _ptr(o["tri_status"]), _ptr(o["wpt"]), _ptr(o["invdepth"]),
                                                            _ptr(o["src_kfid"])))
        self._tkf_pending = None
        return self._tkf_dicts(R, na, o)

    def lastPriors(self, item, n):
        """(prior (n, 2) float32, has_prior (n,) uint8) of item `item` as the last step used them"""
        pri = np.empty((n, 2), np.float32)
        hp = np.empty(n, np.uint8)
        L.check(self.lib.ov2_btracker_last_priors(self.h_trk, int(item), int(n), _ptr(pri), _ptr(hp)))
        return pri, hp

    def lastKeypoints(self, item, n, want_bv=True):
        unpx = np.empty((n, 2), np.float32)
        bv = np.empty((n, 3), np.float64) if want_bv else None
        L.check(self.lib.ov2_btracker_last_keypoints(self.h_trk, int(item), int(n), _ptr(unpx), _ptr(bv) if want_bv else None))
        return unpx, bv

    def describeBRIEF(self, n_active, pts, n):
        """describeBRIEF on the raw frames of the current step, items [0, n_active).  pts: (>= n_active, cap, 2) float32; n: counts
        (len n_active).  -> (desc (n_active, cap, 32) uint8, valid (n_active, cap) bool; slots past n[b] are zero).  Call it before
        the staging set of those frames is uploaded or prepared again."""
        na = int(n_active)
        p = np.asarray(pts, np.float32)
        if p.ndim != 3 or p.shape[0] < na or p.shape[2] != 2:
            raise ValueError("pts must be (>= n_active, cap, 2)")
        cap = p.shape[1]
        p = np.ascontiguousarray(p[:na])
        nn = np.ascontiguousarray(n, np.int32)
        if len(nn) != na:
            raise ValueError("one point count per active item")
        desc = np.zeros((na, cap, L.OV2_BRIEF_BYTES), np.uint8); valid = np.zeros((na, cap), np.uint8)
        L.check(self.lib.ov2_btracker_describe_brief(self.h_trk, na, _ptr(p), _ptr(nn), cap, _ptr(desc), _ptr(valid)))
        return desc, valid.astype(bool)

    def detectSingleScale(self, n_active, ncellsize, cur, ncur, roi, quality, subpix=True):
        """MapManager::extractKeypoints of items [0, n_active) on their current frames.  cur: (batch, n_max, 2); ncur: counts;
        quality: float64 array, one dmaxquality_ per item, updated in place.  -> list of (k, 2) arrays"""
        cap = max(1, 2 * (self.w // ncellsize) * (self.h // ncellsize))
        cur = np.ascontiguousarray(cur, np.float32).reshape(self.batch, self.n_max, 2)
        nc = np.ascontiguousarray(ncur, np.int32)
        q = np.ascontiguousarray(quality, np.float64)
        assert q is quality or np.shares_memory(q, quality), "quality must be a contiguous float64 array (updated in place)"
        out = np.zeros((n_active, cap, 2), np.float32); on = np.zeros(n_active, np.int32)
        r = (C.c_int * 4)(*[int(v) for v in roi])
        L.check(self.lib.ov2_btracker_detect_singlescale(self.h_trk, int(n_active), int(ncellsize), _ptr(cur), _ptr(nc), r, _ptr(q),
                                                         1 if subpix else 0, _ptr(out), cap, _ptr(on)))
        return [out[b, :on[b]].copy() for b in range(n_active)]

    def detectGFTT(self, n_active, params, cur, ncur, nbmax, roi=None, subpix=True):
        """detectGFTT of items [0, n_active) on their current frames.  params: L.GfttParams (FeatureExtractor.gftt_params());
        cur: (batch, n_max, 2); ncur / nbmax: one per active item; roi None or an (h, w) uint8 mask shared by the items.
        -> list of (k, 2) arrays"""
        cur = np.ascontiguousarray(cur, np.float32).reshape(self.batch, self.n_max, 2)
        nc = np.zeros(self.batch, np.int32); nc[:n_active] = np.asarray(ncur, np.int32)[:n_active]
        nb = np.ascontiguousarray(nbmax, np.int32)
        cap = max([1] + [int(v) if v != -1 else params.nmaxpts for v in nb[:n_active]])
        r, rp, rs = _roi_arg(roi, self.w, self.h)
        out = np.zeros((n_active, cap, 2), np.float32); on = np.zeros(n_active, np.int32)
        L.check(self.lib.ov2_btracker_detect_gftt(self.h_trk, int(n_active), rp, rs, C.byref(params), _ptr(cur), _ptr(nc), _ptr(nb),
                                                  1 if subpix else 0, _ptr(out), cap, _ptr(on)))
        return [out[b, :on[b]].copy() for b in range(n_active)]

    def detectGridFAST(self, n_active, ncellsize, cur, ncur, fast_th, mask_mode=L.OV2_MASK_AS_EXECUTED, subpix=True):
        cap = max(1, (self.w // ncellsize) * (self.h // ncellsize))
        cur = np.ascontiguousarray(cur, np.float32).reshape(self.batch, self.n_max, 2)
        nc = np.ascontiguousarray(ncur, np.int32)
        t = np.ascontiguousarray(fast_th, np.int32)
        assert t is fast_th or np.shares_memory(t, fast_th), "fast_th must be a contiguous int32 array (updated in place)"
        out = np.zeros((n_active, cap, 2), np.float32); on = np.zeros(n_active, np.int32)
        L.check(self.lib.ov2_btracker_detect_grid_fast(self.h_trk, int(n_active), int(ncellsize), _ptr(cur), _ptr(nc), _ptr(t), int(mask_mode),
                                                       1 if subpix else 0, _ptr(out), cap, _ptr(on)))
        return [out[b, :on[b]].copy() for b in range(n_active)]

    @property
    def cur_pyr(self):
        """the current frame's pyramids, all items (e.g. `left` of stereo.stereo_match_batch_arrays)"""
        v = _PyrView(self.ctx, C.c_void_p(self.lib.ov2_btracker_cur_pyr(self.h_trk)), self.w, self.h, self.win)
        v.batch = self.batch
        return v

    def cur_item(self, item):
        return _PyrView(self.ctx, C.c_void_p(self.lib.ov2_btracker_cur_item(self.h_trk, int(item))), self.w, self.h, self.win)

    def prev_item(self, item):
        return _PyrView(self.ctx, C.c_void_p(self.lib.ov2_btracker_prev_item(self.h_trk, int(item))), self.w, self.h, self.win)

    # ---- tracking from the keyframe: VisualFrontEnd::kltTrackingFromKF (ov2_btracker_set_track_from_keyframe) ----------------------
    def setTrackFromKeyframe(self, on=True):
        """btrack_keyframetoframe: while on, trackFrameEpiPose, trackMono and trackMonoResident track every frame from the item's last
        keyframe -- its pyramid in the tracker's keyframe store, its px from the keyframe-px table, joined by lmid -- instead of the
        previous frame, and createKeyframe adopts the pyramid and installs the table of every item it creates.  status 4 marks a
        slot the keyframe no longer holds.  The first call allocates the store.  Between steps only."""
        L.check(self.lib.ov2_btracker_set_track_from_keyframe(self.h_trk, 1 if on else 0))

    def adoptKeyframePyramid(self, n_active, do):
        """the current pyramid of every item b < n_active with do[b] becomes its keyframe pyramid (ov2_btracker_adopt_keyframe_pyramid):
        for keyframes built on the host.  Between steps only."""
        d = np.zeros(max(1, int(n_active)), np.uint8)
        d[:int(n_active)] = np.asarray(do, np.uint8).reshape(-1)[:int(n_active)] != 0
        L.check(self.lib.ov2_btracker_adopt_keyframe_pyramid(self.h_trk, int(n_active), _ptr(d)))

    def setKeyframePx(self, item, lmid, px):
        """the keyframe-px table of item `item` (ov2_btracker_set_keyframe_px): lmid (n,) strictly ascending, px (n, 2) finite, the
        keyframe's distorted pixel of every id."""
        lm = np.ascontiguousarray(lmid, np.int32).reshape(-1)
        px = np.ascontiguousarray(px, np.float32).reshape(-1, 2)
        if len(lm) != len(px):
            raise ValueError("one px per lmid")
        L.check(self.lib.ov2_btracker_set_keyframe_px(self.h_trk, int(item), len(lm), _ptr(lm), _ptr(px)))

    def getKeyframePx(self, item, from_device=True):
        """the keyframe-px table of item `item` -> dict(n, lmid (n,), px (n, 2)), from the device or the host mirror"""
        n = C.c_int()
        lm, px = np.zeros(self.n_max, np.int32), np.zeros((self.n_max, 2), np.float32)
        L.check(self.lib.ov2_btracker_get_keyframe_px(self.h_trk, int(item), int(bool(from_device)), C.byref(n), _ptr(lm), _ptr(px)))
        k = n.value
        return dict(n=k, lmid=lm[:k].copy(), px=px[:k].copy())

    def kf_item(self, item):
        """item `item` of the keyframe store as a batch-1 pyramid view (None before the first setTrackFromKeyframe)"""
        h = self.lib.ov2_btracker_kf_item(self.h_trk, int(item))
        return _PyrView(self.ctx, C.c_void_p(h), self.w, self.h, self.win) if h else None

    def close(self):
        if getattr(self, "h_trk", None):
            self.image_buffers = None
            self.lib.ov2_btracker_destroy(self.h_trk)
            self.h_trk = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _gftt_params(nmaxpts, nmaxdist, nmindist, dminquality, dmaxquality):
    return L.GfttParams(int(nmaxpts), int(nmaxdist), int(nmindist), float(dminquality), float(dmaxquality))


def _roi_arg(roi, w, h):
    """roi: None or an (h, w) uint8 mask (any row stride) -> (array or None, pointer, stride)"""
    if roi is None:
        return None, None, 0
    r = np.asarray(roi)
    if r.dtype != np.uint8 or r.ndim != 2 or r.strides[1] != 1 or r.strides[0] < r.shape[1]:
        r = np.ascontiguousarray(r, dtype=np.uint8)
    if r.shape != (h, w):
        raise ValueError("roi must be an (h, w) uint8 mask")
    return r, _ptr(r), r.strides[0]


def set_mask(mask, vpts, dist):
    """FeatureExtractor::setMask (src/feature_extractor.cpp:575-584) in place on an (h, w) uint8 mask: a filled disc of radius dist
    (value 0) at cvRound of every point."""
    if mask.dtype != np.uint8 or mask.ndim != 2 or mask.strides[1] != 1:
        raise ValueError("mask must be a 2-D uint8 array with unit column stride")
    pts = np.ascontiguousarray(vpts, dtype=np.float32).reshape(-1, 2)
    h, w = mask.shape
    L.check(L.load().ov2_set_mask(mask.ctypes.data_as(C.c_void_p), w, h, mask.strides[0], _ptr(pts), len(pts), int(dist)))
    return mask


class FeatureExtractor:
    """Mirror of /root/reference/include/feature_extractor.hpp:30-54: holds the
    adaptive thresholds nfast_th_ and dmaxquality_ that the two grid detectors update, and detectGFTT's
    nmaxpts_ / nmaxdist_ / nmindist_ / dminquality_ (derived like the constructor, :79-83, unless given)."""

    def __init__(self, ctx, nfast_th=10, dmaxquality=0.001, mask_mode=L.OV2_MASK_AS_EXECUTED, nmaxpts=300, nmaxdist=35,
                 nmindist=None, dminquality=None):
        self.ctx, self.lib = ctx, ctx.lib
        self.nfast_th_ = int(nfast_th)
        self.dmaxquality_ = float(dmaxquality)
        self.mask_mode = mask_mode
        self.nmaxpts_ = int(nmaxpts)
        self.nmaxdist_ = int(nmaxdist)
        self.nmindist_ = int(nmaxdist) // 2 if nmindist is None else int(nmindist)
        self.dminquality_ = float(dmaxquality) / 2. if dminquality is None else float(dminquality)

    def gftt_params(self):
        return _gftt_params(self.nmaxpts_, self.nmaxdist_, self.nmindist_, self.dminquality_, self.dmaxquality_)

    def _gftt_cap(self, ncur, nbmax):
        return max(1, int(nbmax) if nbmax != -1 else self.nmaxpts_ - ncur)

    def detectGFTT(self, im, vcurkps, roi=None, nbmax=-1, subpix=True):
        """src/feature_extractor.cpp:104-221 on a host image (any row stride).  roi: None or an (h, w) uint8 mask."""
        im = np.asarray(im)
        if im.dtype != np.uint8 or im.ndim != 2 or im.strides[1] != 1 or im.strides[0] < im.shape[1]:
            im = np.ascontiguousarray(im, dtype=np.uint8)
        if im.size == 0:
            return np.zeros((0, 2), np.float32)
        h, w = im.shape
        cur = np.ascontiguousarray(vcurkps, dtype=np.float32).reshape(-1, 2)
        r, rp, rs = _roi_arg(roi, w, h)
        cap = self._gftt_cap(len(cur), nbmax)
        out = np.zeros((cap, 2), np.float32)
        n = C.c_int(0)
        p = self.gftt_params()
        L.check(self.lib.ov2_detect_gftt(self.ctx.h, _ptr(im), w, h, im.strides[0], rp, rs, C.byref(p), _ptr(cur), len(cur),
                                         int(nbmax), int(bool(subpix)), _ptr(out), cap, C.byref(n)))
        return out[:n.value].copy()

    def detectGFTTPyr(self, pyr, vcurkps, roi=None, nbmax=-1, subpix=True, item=0):
        """detectGFTT on level 0 of a device-resident pyramid (the CLAHE'd cur_img_ of the keyframe) -- no image upload."""
        cur = np.ascontiguousarray(vcurkps, dtype=np.float32).reshape(-1, 2)
        w, h = pyr.level_size(0)
        r, rp, rs = _roi_arg(roi, w, h)
        cap = self._gftt_cap(len(cur), nbmax)
        out = np.zeros((cap, 2), np.float32)
        n = C.c_int(0)
        p = self.gftt_params()
        L.check(self.lib.ov2_detect_gftt_d(self.ctx.h, pyr.h_pyr, int(item), rp, rs, C.byref(p), _ptr(cur), len(cur),
                                           int(nbmax), int(bool(subpix)), _ptr(out), cap, C.byref(n)))
        return out[:n.value].copy()

    @staticmethod
    def detectGFTTBatch(ctx, pyr, roi_d, roi_stride, params, cur_xy_d, cur_cap, ncur_d, nbmax, out_xy_d, out_cap, subpix=True):
        """ov2_detect_gftt_batch_d: detectGFTT on EVERY batch item of `pyr`.  roi_d / cur_xy_d / ncur_d / out_xy_d are device
        addresses (ints; 0 = NULL for the first three); params an L.GfttParams (FeatureExtractor.gftt_params()); nbmax one int
        per item.  Returns the per-item point counts (int32 array)."""
        nb = np.ascontiguousarray(nbmax, np.int32)
        if len(nb) != pyr.batch:
            raise ValueError("one nbmax per batch item")
        n = np.zeros(pyr.batch, np.int32)
        L.check(ctx.lib.ov2_detect_gftt_batch_d(ctx.h, pyr.h_pyr, C.c_void_p(roi_d or None), int(roi_stride), C.byref(params),
                                                C.c_void_p(cur_xy_d or None), int(cur_cap), C.c_void_p(ncur_d or None), _ptr(nb),
                                                1 if subpix else 0, C.c_void_p(out_xy_d), int(out_cap), n.ctypes.data_as(C.c_void_p)))
        return n

    def setMask(self, im, vpts, dist, mask=None):
        """src/feature_extractor.cpp:575-584: mask None -> a new all-255 (h, w) mask; returns the mask."""
        if mask is None:
            h, w = np.asarray(im).shape[:2]
            mask = np.full((h, w), 255, np.uint8)
        return set_mask(mask, vpts, dist)

    def detectGridFAST(self, im, ncellsize, vcurkps, roi=None, subpix=True):
        """src/feature_extractor.cpp:443-570 (roi is unused there too)."""
        im = np.ascontiguousarray(im, dtype=np.uint8)
        if im.size == 0:
            return np.zeros((0, 2), np.float32)               # :446-449
        h, w = im.shape
        cur = np.ascontiguousarray(vcurkps, dtype=np.float32).reshape(-1, 2)
        cap = max(1, (w // ncellsize) * (h // ncellsize))
        out = np.zeros((cap, 2), np.float32)
        n = C.c_int(0)
        th = C.c_int(self.nfast_th_)
        L.check(self.lib.ov2_detect_grid_fast(self.ctx.h, _ptr(im), w, h, w, int(ncellsize), _ptr(cur), cur.shape[0],
                                              C.byref(th), self.mask_mode, int(bool(subpix)), _ptr(out), C.byref(n)))
        self.nfast_th_ = th.value
        return out[:n.value].copy()

    def detectSingleScale(self, im, ncellsize, vcurkps, roi, subpix=True):
        """src/feature_extractor.cpp:288-440.  roi = (x, y, width, height)."""
        im = np.ascontiguousarray(im, dtype=np.uint8)
        if im.size == 0:
            return np.zeros((0, 2), np.float32)               # :291-294
        h, w = im.shape
        cur = np.ascontiguousarray(vcurkps, dtype=np.float32).reshape(-1, 2)
        cap = max(1, 2 * (w // ncellsize) * (h // ncellsize))
        out = np.zeros((cap, 2), np.float32)
        n = C.c_int(0)
        q = C.c_double(self.dmaxquality_)
        roi_a = (C.c_int * 4)(*[int(v) for v in roi])
        L.check(self.lib.ov2_detect_singlescale(self.ctx.h, _ptr(im), w, h, w, int(ncellsize), _ptr(cur), cur.shape[0],
                                                roi_a, C.byref(q), int(bool(subpix)), _ptr(out), C.byref(n)))
        self.dmaxquality_ = q.value
        return out[:n.value].copy()

    def detectSingleScalePyr(self, pyr, ncellsize, vcurkps, roi, subpix=True, item=0):
        """detectSingleScale on level 0 of a device-resident pyramid (e.g. VisualFrontEndTracker.cur_pyr: the CLAHE'd
        cur_img_ of the keyframe, src/map_manager.cpp:312-320) -- no image upload."""
        cur = np.ascontiguousarray(vcurkps, dtype=np.float32).reshape(-1, 2)
        w, h = pyr.level_size(0)
        out = np.zeros((max(1, 2 * (w // ncellsize) * (h // ncellsize)), 2), np.float32)
        n = C.c_int(0); q = C.c_double(self.dmaxquality_)
        roi_a = (C.c_int * 4)(*[int(v) for v in roi])
        L.check(self.lib.ov2_detect_singlescale_d(self.ctx.h, pyr.h_pyr, int(item), int(ncellsize), _ptr(cur), cur.shape[0],
                                                  roi_a, C.byref(q), int(bool(subpix)), _ptr(out), C.byref(n)))
        self.dmaxquality_ = q.value
        return out[:n.value].copy()

    @staticmethod
    def detectSingleScaleBatch(ctx, pyr, ncellsize, cur_xy_d, cur_cap, ncur_d, roi, quality, out_xy_d, out_cap, subpix=True):
        """ov2_detect_singlescale_batch_d: detectSingleScale on EVERY batch item of `pyr` in one call.  cur_xy_d / ncur_d /
        out_xy_d are device addresses (ints; 0 = NULL for the first two), `quality` a float64 array with one dmaxquality_ per
        item (updated in place like the member).  Returns the per-item point counts (int32 array)."""
        q = np.ascontiguousarray(quality, np.float64)
        assert q is quality or np.shares_memory(q, quality), "quality must be a contiguous float64 array (updated in place)"
        n = np.zeros(pyr.batch, np.int32)
        r = (C.c_int * 4)(*[int(v) for v in roi])
        L.check(ctx.lib.ov2_detect_singlescale_batch_d(ctx.h, pyr.h_pyr, int(ncellsize), C.c_void_p(cur_xy_d or None), int(cur_cap),
                                                       C.c_void_p(ncur_d or None), r, q.ctypes.data_as(C.c_void_p), 1 if subpix else 0,
                                                       C.c_void_p(out_xy_d), int(out_cap), n.ctypes.data_as(C.c_void_p)))
        return n

    @staticmethod
    def detectGridFASTBatch(ctx, pyr, ncellsize, cur_xy_d, cur_cap, ncur_d, fast_th, out_xy_d, out_cap, mask_mode=L.OV2_MASK_AS_EXECUTED, subpix=True):
        """ov2_detect_grid_fast_batch_d; `fast_th` an int32 array with one nfast_th_ per item (updated in place)."""
        t = np.ascontiguousarray(fast_th, np.int32)
        assert t is fast_th or np.shares_memory(t, fast_th), "fast_th must be a contiguous int32 array (updated in place)"
        n = np.zeros(pyr.batch, np.int32)
        L.check(ctx.lib.ov2_detect_grid_fast_batch_d(ctx.h, pyr.h_pyr, int(ncellsize), C.c_void_p(cur_xy_d or None), int(cur_cap),
                                                     C.c_void_p(ncur_d or None), t.ctypes.data_as(C.c_void_p), int(mask_mode), 1 if subpix else 0,
                                                     C.c_void_p(out_xy_d), int(out_cap), n.ctypes.data_as(C.c_void_p)))
        return n

    def detectGridFASTPyr(self, pyr, ncellsize, vcurkps, subpix=True, item=0):
        """detectGridFAST on level 0 of a device-resident pyramid."""
        cur = np.ascontiguousarray(vcurkps, dtype=np.float32).reshape(-1, 2)
        w, h = pyr.level_size(0)
        out = np.zeros((max(1, (w // ncellsize) * (h // ncellsize)), 2), np.float32)
        n = C.c_int(0); th = C.c_int(self.nfast_th_)
        L.check(self.lib.ov2_detect_grid_fast_d(self.ctx.h, pyr.h_pyr, int(item), int(ncellsize), _ptr(cur), cur.shape[0],
                                                C.byref(th), self.mask_mode, int(bool(subpix)), _ptr(out), C.byref(n)))
        self.nfast_th_ = th.value
        return out[:n.value].copy()

    def describeBRIEF(self, im, vpts):
        """src/feature_extractor.cpp:224-285 (BriefDescriptorExtractor, 32 bytes) with the context's pattern (Context.set_brief_pattern).
        im: (h, w) uint8, any row stride.  -> (desc (n, 32) uint8, valid (n,) bool): the reference's empty cv::Mat of a point too
        close to the border is valid False (its row is zero)."""
        im = np.asarray(im)
        if im.dtype != np.uint8 or im.ndim != 2 or im.strides[1] != 1 or im.strides[0] < im.shape[1]:
            im = np.ascontiguousarray(im, dtype=np.uint8)
        h, w = im.shape
        pts = np.ascontiguousarray(vpts, dtype=np.float32).reshape(-1, 2)
        n = len(pts)
        desc = np.zeros((n, L.OV2_BRIEF_BYTES), np.uint8); valid = np.zeros(n, np.uint8)
        L.check(self.lib.ov2_describe_brief(self.ctx.h, _ptr(im), w, h, im.strides[0], _ptr(pts), n, _ptr(desc), _ptr(valid)))
        return desc, valid.astype(bool)

    @staticmethod
    def describeBRIEFBatch(ctx, img_d, w, h, pitch, item_stride, n_items, xy_d, cap, n_d, desc_d, valid_d):
        """ov2_describe_brief_batch_d: every argument a device address (int) or size; n_d may be 0 (all cap slots)."""
        L.check(ctx.lib.ov2_describe_brief_batch_d(ctx.h, C.c_void_p(img_d), int(w), int(h), int(pitch), int(item_stride), int(n_items),
                                                   C.c_void_p(xy_d), int(cap), C.c_void_p(n_d or None), C.c_void_p(desc_d), C.c_void_p(valid_d)))

    def cornerSubPix(self, im, pts, half_win=3, max_iter=30, eps=0.01):
        im = np.ascontiguousarray(im, dtype=np.uint8)
        h, w = im.shape
        p = np.array(pts, dtype=np.float32, copy=True).reshape(-1, 2)
        if p.shape[0]:
            L.check(self.lib.ov2_corner_subpix(self.ctx.h, _ptr(im), w, h, w, _ptr(p), p.shape[0], half_win, max_iter, eps))
        return p


class CameraCalibration:
    """Mirror of the reference's CameraCalibration / Frame::computeKeypoint pair
    (/root/reference/src/camera_calibration.cpp:313-333, src/frame.cpp:246-254) for arrays of keypoints.

    model: "pinhole" | "fisheye"; K = (fx, fy, cx, cy); D = distortion coefficients or None
    (`Dcv_.empty()` -> undistortImagePoint returns the point unchanged)."""

    MODELS = {"pinhole": L.OV2_CAM_PINHOLE, "fisheye": L.OV2_CAM_FISHEYE}

    def __init__(self, ctx, model, fx, fy, cx, cy, D=None):
        self.ctx, self.lib = ctx, ctx.lib
        self.model = self.MODELS[model]
        self.K = np.array([fx, fy, cx, cy], np.float64)
        self.D = None if D is None or len(D) == 0 else np.ascontiguousarray(D, dtype=np.float64)
        Km = np.array([[fx, 0., cx], [0., fy, cy], [0., 0., 1.]])
        self.iK = np.ascontiguousarray(np.linalg.inv(Km))            # the reference's iK_ = K_.inverse()

    def computeKeypoints(self, px, want_bv=True):
        """px (n,2) float32 -> (unpx (n,2) float32, bv (n,3) float64 or None)."""
        px = np.ascontiguousarray(px, dtype=np.float32).reshape(-1, 2)
        n = len(px)
        unpx = np.empty((n, 2), np.float32)
        bv = np.empty((n, 3), np.float64) if want_bv else None
        L.check(self.lib.ov2_compute_keypoints(self.ctx.h, self.model, _ptr(self.K), _ptr(self.D) if self.D is not None else None,
                                               0 if self.D is None else len(self.D), _ptr(self.iK), _ptr(px), n, _ptr(unpx),
                                               _ptr(bv) if want_bv else None))
        return unpx, bv

    def undistortImagePoint(self, pt):
        return self.computeKeypoints(np.asarray(pt, np.float32).reshape(1, 2), want_bv=False)[0][0]

    def setRectifyMaps(self, form, map1, map2):
        """The maps of setUndistMap ("f32") / setUndistStereoMap ("fixed") (src/camera_calibration.cpp:92-97, :141-145), computed by the
        caller once at start-up; as there, the calibration is the rectified one from then on (D_ empty).  -> the RectifyMap"""
        self.rectify_map = RectifyMap(self.ctx, form, map1, map2)
        self.D = None
        return self.rectify_map

    def rectifyImage(self, img, out=None):
        """src/camera_calibration.cpp:233-241: cv::remap through the maps when they are set, the image itself otherwise"""
        rm = getattr(self, "rectify_map", None)
        if rm is None:
            return img
        return rm.rectify(img, out)
