"""What LockstepTracker hands the C ABI, without a GPU: the tracker runs over a stub library that records every ov2_* call and decodes,
while the call is in flight, every array and struct its arguments point at.  For every call family, whole and Begin + End: the entry
point and its argument count (L.SIGNATURES), the bytes of every input in the dtype, shape and order include/ov2slam_hip.h gives it,
the fields of the params / input structs (the NULLs of the resident forms among them), the whole call's arguments being the _begin
arguments followed by the _end arguments, and the arity, shapes and dtypes of what Python returns.  Then the rules around the one open
call: a refused call changes nothing an End or a last*Inputs reads, and an End with nothing open reaches the library."""
import ctypes as C
import weakref

import numpy as np
import pytest

from ov2slam_amd import LockstepTracker, Ov2Error
from ov2slam_amd import _lib as L

B, NA, W, H, N = 3, 2, 64, 48, 8
BN = B * N
HPYR = 0x5A5A00


def _a(nbytes):
    return ("a", nbytes)


_MAP = ["i", "imgs", "i", _a(BN * 8), _a(BN * 24), _a(BN), _a(NA * 56), _a(NA * 4), "i"]
_STEP_END = [_a(BN * 8), _a(BN), _a(NA * 4)]
BEGIN = {"track_frame": ["i", "imgs", "i", _a(BN * 8), _a(BN * 8), _a(BN), _a(NA * 4), "i"],
         "track_frame_map": _MAP, "track_frame_pose": _MAP + ["s", "s"], "track_frame_epi_pose": _MAP + ["s", "s"],
         "track_mono": ["i", "imgs", "i", _a(BN * 8), _a(BN * 24), _a(BN), _a(NA * 4), "i", "s", "s"],
         "track_mono_resident": ["i", "imgs", "i", "i", "s", "s"],
         "create_keyframe": ["i", "s", "s"], "stereo_keyframe": ["i", "s", "i", _a(NA)], "temporal_keyframe": ["i", "s", _a(NA)]}
END = {"track_frame": _STEP_END, "track_frame_pose": _STEP_END + ["r"], "track_frame_epi_pose": _STEP_END + ["r", "r"],
       "track_mono": _STEP_END + ["r", "r", "r"], "track_mono_resident": _STEP_END + ["r", "r", "r", "r"],
       "create_keyframe": ["r", _a(BN * 8), _a(BN * 4), _a(BN * 8), _a(BN * 24), _a(BN * 32), _a(BN), _a(BN)],
       "stereo_keyframe": ["r", _a(BN * 8), _a(BN), _a(BN), _a(BN * 24), _a(BN * 8)],
       "temporal_keyframe": ["r", _a(BN), _a(BN * 24), _a(BN * 8), _a(BN * 4)]}
END_OF = dict({f: f for f in END}, track_frame_map="track_frame")             # (trackFrameMap has no end call of its own)
# bytes behind every pointer field of the input and result structs (0: only NULL or not is recorded)
POINTEE = dict(Twc_h=NA * 56, scale_h=BN * 4, p3p_req_h=NA, seed_h=NA * 8, lmid_h=BN * 4, nbkfs_h=NA * 4, epi_seed_h=NA * 8, time_h=NA * 8,
               frame_id_h=NA * 4, localba_is_on_h=NA, px_h=BN * 8, is3d_h=BN, n_h=NA * 4, make_kf_h=NA, nlmid_h=NA * 4, nkfid_h=NA * 4,
               quality_inout=NA * 8, fast_th_inout=NA * 4, removed=N, pair_cur=N * 4, err=N * 4, trace_samples=0, D=0)


def _addr(a):
    if a is None or isinstance(a, int):
        return a
    if isinstance(a, C.c_void_p):
        return a.value
    if isinstance(a, C._Pointer):
        return C.cast(a, C.c_void_p).value
    return C.addressof(a)


def _walk(s, prefix=""):
    """a ctypes struct -> {path: value}, every pointer field replaced by the bytes behind it (None: NULL)"""
    d = {}
    for name, _ in s._fields_:
        v = getattr(s, name)
        if isinstance(v, C.Structure):
            d.update(_walk(v, prefix + name + "."))
        elif isinstance(v, C._Pointer):
            p = _addr(v)
            d[prefix + name] = None if not p else (C.string_at(p, POINTEE[name]) if POINTEE[name] else "set")
        elif isinstance(v, C.Array):
            d[prefix + name] = [_walk(x) if isinstance(x, C.Structure) else x for x in v]
        else:
            d[prefix + name] = v
    return d


def _decode(kind, a):
    if kind == "i":
        return _addr(a)
    if kind == "imgs":
        return [C.string_at(p, H * W) for p in a]
    if kind == "s":
        return _walk(a._obj if hasattr(a, "_obj") else a)
    if kind == "r":
        return None if a is None else (type(a[0]).__name__, len(a), [_walk(x) for x in a])
    p = _addr(a)
    return None if not p else C.string_at(p, kind[1])


def _spec(name):
    stem = name[len("ov2_btracker_"):]
    if stem.endswith("_begin"):
        return BEGIN.get(stem[:-6])
    if stem.endswith("_end"):
        return END.get(stem[:-4])
    return BEGIN[stem] + END[END_OF[stem]] if stem in BEGIN else None


class _Lib:
    """answers every ov2_* with a function that records (name, decoded arguments) and returns OV2_OK, or `refuse[name]`"""

    def __init__(self):
        self.calls, self.refuse, self.table_rows = [], {}, 0
        self.slot = (C.c_uint8 * (H * W))()

    def __getattr__(self, name):
        if not name.startswith("ov2_"):
            raise AttributeError(name)

        def fn(*args):
            if name == "ov2_btracker_image_buffer":
                args[3]._obj.value = W
                return C.addressof(self.slot)
            spec = _spec(name)
            if spec is not None:
                assert len(args) == 1 + len(spec) == len(L.SIGNATURES[name][1]), name
                self.calls.append((name, [_decode(k, a) for k, a in zip(spec, args[1:])]))
            else:
                self.calls.append((name, args))
            if name in ("ov2_btracker_last_pose_inputs", "ov2_btracker_last_epi_inputs") and name not in self.refuse:
                cols = 4 if "pose" in name else 8
                tab, rows = args[-2], args[-1]._obj
                for i in range(self.table_rows * cols):
                    tab[i] = 1000 + i
                rows.value = self.table_rows
            return self.refuse.get(name, L.OV2_OK)
        return fn


class _Ctx:
    def __init__(self):
        self.lib, self.h, self._children = _Lib(), C.c_void_p(1), weakref.WeakSet()


class _Pyr:
    h_pyr = C.c_void_p(HPYR)


def _tracker():
    ctx = _Ctx()
    t = LockstepTracker(ctx, B, W, H, use_clahe=False, nbmaxkps=N)
    assert t.stride == W and t.image_buffers[2][B - 1].shape == (H, W)
    del ctx.lib.calls[:]
    return t, ctx.lib


def _b(x, dt):
    return np.ascontiguousarray(x, dt).tobytes()


def _inputs():
    """the public arguments, in dtypes and containers that marshalling has to convert"""
    r = np.random.default_rng(7)
    x = dict(imgs=[r.integers(0, 255, (H, W), dtype=np.uint8) for _ in range(NA)], kps=r.random((B, N, 2)) * 50, pri=r.random((B, N, 2)) * 50,
             hasprior=r.integers(0, 2, (B, N)), n=[5, 7], wpt=r.random((B, N, 3)).astype(np.float32), is3d=r.integers(0, 2, (B, N)) > 0,
             Tcw=r.random((NA, 7)), Twc=r.random((NA, 7)), p3p_req=[1, 0], seed=[11, 2 ** 63 + 5], scale=r.integers(0, 4, (B, N)),
             lmid=r.integers(0, 999, (B, N)), nbkfs=[3, 4], epi_seed=[5, 6], time=[1.5, 2.5], frame_id=[7, 8], ba=[1, 0],
             px=r.random((B, N, 2)) * 50, make_kf=[1, 0], nlmid=[100, 200], nkfid=[3, 4], do=[0, 1], state=np.array([0.5, 0.25]))
    x["pp"], x["ep"] = L.PoseParams(), L.EpifilterParams()
    x["pp"].mono, x["ep"].n_rows, x["ep"].mono, x["ep"].fransac_err = 1, 48, 1, 3.0
    x["ckf"] = dict(ncellsize=16, nbwcells=4, nbhcells=3, nbmaxkps=N, detector="singlescale", det_cell=16, roi=(1, 2, 60, 40), mask_mode=0,
                    do_subpix=False, use_brief=True)
    x["skf"], x["tkf"] = L.StereoKeyframeParams(), L.TemporalKeyframeParams()
    x["skf"].ncellsize, x["tkf"].n_src_max = 16, 5
    return x


X = _inputs()
_IMGS = [im.tobytes() for im in X["imgs"]]
_MAPV = [NA, _IMGS, W, _b(X["kps"], np.float32), _b(X["wpt"], np.float64), _b(X["is3d"], np.uint8), _b(X["Tcw"], np.float64), _b(X["n"], np.int32), 1]
_POSE_IN = dict(Twc_h=_b(X["Twc"], np.float64), scale_h=_b(X["scale"], np.int32), p3p_req_h=_b(X["p3p_req"], np.uint8),
                seed_h=_b(X["seed"], np.uint64))
_EPI_IN = dict({"pose." + k: v for k, v in _POSE_IN.items()}, lmid_h=_b(X["lmid"], np.int32), nbkfs_h=_b(X["nbkfs"], np.int32),
               epi_seed_h=_b(X["epi_seed"], np.uint64))
_MONO_IN = dict({"step." + k: v for k, v in _EPI_IN.items()}, time_h=_b(X["time"], np.float64), frame_id_h=_b(X["frame_id"], np.int32),
                localba_is_on_h=_b(X["ba"], np.uint8))
_MONO_IN["step.pose.Twc_h"] = None                                            # the pose is resident
_RES_IN = dict(_MONO_IN, **{"step.lmid_h": None, "step.pose.scale_h": None})  # ... and so are the frame and its scales
_POSE_P = dict({"pose." + k: v for k, v in _walk(X["pp"]).items()}, dop3p=1, n_rows=64)
_EPI_P = dict({"pose." + k: v for k, v in _POSE_P.items()}, **{"epi." + k: v for k, v in _walk(X["ep"]).items()})
_MONO_P = dict({"step." + k: v for k, v in _EPI_P.items()}, doepipolar=1)
_CKF_P = dict(ncellsize=16, nbwcells=4, nbhcells=3, nbmaxkps=N, detector=L.OV2_CKF_DET_SINGLESCALE, det_cell=16, roi=[1, 2, 60, 40], mask_mode=0,
              do_subpix=0, use_brief=1)
_CKF_IN = dict(px_h=_b(X["px"], np.float32), lmid_h=_b(X["lmid"], np.int32), is3d_h=_b(X["is3d"], np.uint8), n_h=_b(X["n"], np.int32),
               make_kf_h=_b(X["make_kf"], np.uint8), nlmid_h=_b(X["nlmid"], np.int32), nkfid_h=_b(X["nkfid"], np.int32),
               time_h=_b(X["time"], np.float64), Twc_h=_b(X["Twc"], np.float64), quality_inout=_b(X["state"], np.float64), fast_th_inout=None)
_CKF_RES = dict(_CKF_IN, px_h=None, lmid_h=None, is3d_h=None, n_h=None, Twc_h=None)
_POSE_A = (X["imgs"], X["kps"], X["wpt"], X["is3d"], X["Tcw"], X["n"], X["pp"], X["Twc"], X["p3p_req"], X["seed"])
_EPI_A = _POSE_A[:7] + (X["ep"],) + _POSE_A[7:] + (X["lmid"], X["nbkfs"], X["epi_seed"])
_MONO_A = (X["imgs"], X["kps"], X["wpt"], X["is3d"], X["n"], X["pp"], X["ep"], X["p3p_req"], X["seed"], X["lmid"], X["nbkfs"], X["epi_seed"],
           X["time"], X["frame_id"])
_RES_A = (X["imgs"],) + _MONO_A[5:9] + _MONO_A[10:]
_POSE_KW = dict(scale=X["scale"], dop3p=True, n_rows=64)
_MONO_V = [NA, _IMGS, W, _MAPV[3], _MAPV[4], _MAPV[5], _MAPV[7], 1]
_ZERO_TCW = [NA, _IMGS, W, _MAPV[3], _MAPV[4], _MAPV[5], bytes(NA * 56), _MAPV[7], 1]

# family -> (method stem, args, kwargs, the _begin arguments as the header lays them out, arity of the return value)
CASES = {
    "track_frame": ("trackFrame", (X["imgs"], X["kps"], X["pri"], X["hasprior"], X["n"]), dict(klt_use_prior=False),
                    [NA, _IMGS, W, _b(X["kps"], np.float32), _b(X["pri"], np.float32), _b(X["hasprior"], np.uint8), _b(X["n"], np.int32), 0], 3),
    "track_frame_nohp": ("trackFrame", (X["imgs"], X["kps"], X["pri"], None, X["n"]), {},
                         [NA, _IMGS, W, _b(X["kps"], np.float32), _b(X["pri"], np.float32), None, _b(X["n"], np.int32), 1], 3),
    "track_frame_map": ("trackFrameMap", _POSE_A[:6], {}, _MAPV, 3),
    "track_frame_pose": ("trackFramePose", _POSE_A, _POSE_KW, _MAPV + [_POSE_P, _POSE_IN], 4),
    "track_frame_epi_pose": ("trackFrameEpiPose", _EPI_A, _POSE_KW, _MAPV + [_EPI_P, _EPI_IN], 5),
    "track_mono": ("trackMono", _MONO_A, dict(_POSE_KW, localba_is_on=X["ba"]), _MONO_V + [_MONO_P, _MONO_IN], 6),
    "track_mono_noepi": ("trackMono", _MONO_A, dict(_POSE_KW, localba_is_on=X["ba"], doepipolar=False),
                         _MONO_V + [dict(_MONO_P, doepipolar=0), _MONO_IN], 6),
    "track_mono_resident": ("trackMonoResident", _RES_A, dict(localba_is_on=X["ba"], dop3p=True, n_rows=64),
                            [NA, _IMGS, W, 1, _MONO_P, _RES_IN], 7),
    "create_keyframe": ("createKeyframe", (NA, X["px"], X["lmid"], X["is3d"], X["n"], X["make_kf"], X["nlmid"], X["nkfid"], X["time"], X["ckf"],
                                           X["state"]), dict(Twc=X["Twc"]), [NA, _CKF_P, _CKF_IN], 2),
    "create_keyframe_resident": ("createKeyframe", (NA, None, None, None, None, X["make_kf"], X["nlmid"], X["nkfid"], X["time"], X["ckf"],
                                                    X["state"]), {}, [NA, _CKF_P, _CKF_RES], 2),
    "stereo_keyframe": ("stereoKeyframe", (NA, _Pyr(), X["do"], X["skf"]), {}, [NA, _walk(X["skf"]), HPYR, _b(X["do"], np.uint8)], 2),
    "temporal_keyframe": ("temporalKeyframe", (NA, X["do"], X["tkf"]), {}, [NA, _walk(X["tkf"]), _b(X["do"], np.uint8)], 2),
}


def _describe(v):
    """a return value -> its structure: container types, array shapes and dtypes, and that nothing in it is non-zero"""
    if isinstance(v, np.ndarray):
        return ("array", v.shape, v.dtype.str, bool(v.any()))
    if isinstance(v, dict):
        return {k: _describe(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return (type(v).__name__, [_describe(x) for x in v])
    return (type(v).__name__, v)


def _matches(got, want):
    if isinstance(want, dict):
        return all(got[k] == v for k, v in want.items())
    return got == want


def _begin_end_of(case):
    fam = case if case in BEGIN else case.rsplit("_", 1)[0]
    return "ov2_btracker_%s" % fam, "ov2_btracker_%s_end" % END_OF[fam]


@pytest.mark.parametrize("case", sorted(CASES))
def test_whole_and_halves_marshal_alike(case):
    stem, args, kw, want, arity = CASES[case]
    whole_name, end_name = _begin_end_of(case)
    t, lib = _tracker()
    kf = "keyframe" in case
    state = X["state"].copy()
    if case.startswith("create"):
        args = args[:10] + (state,)
    got_whole = getattr(t, stem)(*args, **kw)
    (name, wargs), = lib.calls
    assert name == whole_name
    del lib.calls[:]
    assert getattr(t, stem + "Begin")(*args, **kw) is None
    end = "trackFrameEnd" if stem == "trackFrameMap" else stem + "End"
    got_split = getattr(t, end)()
    (bname, bargs), (ename, eargs) = lib.calls
    assert bname == whole_name + "_begin" and ename == end_name
    for i, (g, w) in enumerate(zip(bargs, want)):
        assert _matches(g, w), (case, i)
    assert len(bargs) == len(want) and wargs == bargs + eargs                 # the whole call: _begin's arguments, then _end's
    # the result side: zeroed buffers of the header's sizes, per-item structs whose pointers are set (no trace table)
    for a in eargs:
        if isinstance(a, tuple):
            assert a[1] == NA and all(v is not None for r in a[2] for k, v in r.items() if k in ("removed", "pair_cur", "err"))
            assert all(r.get("trace_samples") is None for r in a[2])
        else:
            assert a is None and case == "track_mono_noepi" or a == bytes(len(a))
    assert _describe(got_whole) == _describe(got_split) and len(got_whole) == arity
    if kf:
        records, out = got_whole
        assert len(records) == NA and all(type(v) is int for r in records for v in r.values())
        shapes = {k: (v.shape, v.dtype) for k, v in out.items()}
        assert shapes == {"create": dict(px=((B, N, 2), np.float32), lmid=((B, N), np.int32), unpx=((B, N, 2), np.float32), bv=((B, N, 3), np.float64),
                                         desc=((B, N, 32), np.uint8), valid=((B, N), np.uint8), color=((B, N), np.uint8)),
                          "stereo": dict(right_px=((B, N, 2), np.float32), stereo_ok=((B, N), np.uint8), tri_status=((B, N), np.uint8),
                                         wpt=((B, N, 3), np.float64), invdepth=((B, N), np.float64)),
                          "temporal": dict(tri_status=((B, N), np.uint8), wpt=((B, N, 3), np.float64), invdepth=((B, N), np.float64),
                                           src_kfid=((B, N), np.int32))}[case.split("_")[0]]
        assert set(records[0]) == {"create": {"action", "n_prev", "noccupcells", "nb2detect", "n_new", "n_kf", "nb3dkps"},
                                   "stereo": {f for f, _ in L.StereoKeyframeResult._fields_},
                                   "temporal": {f for f, _ in L.TemporalKeyframeResult._fields_}}[case.split("_")[0]]
        return
    out, st, p3p = got_whole[:3]
    assert (out.shape, out.dtype, st.shape, st.dtype, p3p.shape, p3p.dtype) == ((B, N, 2), np.float32, (B, N), np.uint8, (NA,), np.bool_)
    n = [0, 0] if "resident" in case else X["n"]
    if arity >= 4:
        poses = got_whole[3 + (arity >= 5)]
        assert len(poses) == NA and [p["removed"].shape for p in poses] == [(k,) for k in n] and poses[0]["Twc"].shape == (7,)
    if arity >= 5:
        epis = got_whole[3]
        if case == "track_mono_noepi":
            assert epis is None
        else:
            assert [(e["removed"].shape, e["err"].shape, e["err"].dtype, e["pair_cur"].shape) for e in epis] == [((k,), (k,), np.float32, (0,)) for k in n]
    if arity >= 6:
        assert len(got_whole[5]) == NA and set(got_whole[5][0]) == {"Twc_pred", "resynced", "state", "kf"} and got_whole[5][0]["Twc_pred"].shape == (7,)
    if arity == 7:
        assert got_whole[6] == [dict(n_before=0, n_after=0)] * NA


def test_scatter_into_the_callers_arrays():
    """out[k] of a keyframe call is handed to the library as it is; a wrong one is refused in words, before the library is called"""
    t, lib = _tracker()
    mine = np.full((B, N, 3), 2.5)
    records, out = t.temporalKeyframe(NA, X["do"], X["tkf"], out=dict(wpt=mine))
    assert out["wpt"] is mine and lib.calls[0][1][5] == mine.tobytes()
    t.temporalKeyframeBegin(NA, X["do"], X["tkf"])
    assert t.temporalKeyframeEnd(out=dict(wpt=mine))[1]["wpt"] is mine
    del lib.calls[:]
    with pytest.raises(ValueError) as e:
        t.stereoKeyframe(NA, _Pyr(), X["do"], X["skf"], out=dict(wpt=np.zeros((B, N, 3), np.float32)))
    assert str(e.value) == "out['wpt'] must be a contiguous float64 array of shape (%d, %d, 3)" % (B, N) and not lib.calls


def test_trackFrameEnd_finishes_every_step_form():
    t, lib = _tracker()
    for case in ("track_frame_pose", "track_frame_epi_pose", "track_mono", "track_mono_resident"):
        stem, args, kw, _, _ = CASES[case]
        getattr(t, stem + "Begin")(*args, **kw)
        out, st, p3p = t.trackFrameEnd()
        assert lib.calls[-1][0] == "ov2_btracker_track_frame_end" and p3p.shape == (NA,) and p3p.dtype == np.bool_


def _mono(t, how, **kw):
    stem, args, kw0, _, _ = CASES["track_mono"]
    return getattr(t, stem + how)(*args, **dict(kw0, **kw))


def test_a_refused_begin_leaves_the_open_step_as_it_was():
    t, lib = _tracker()
    _mono(t, "Begin", doepipolar=True)
    lib.refuse["ov2_btracker_track_mono_begin"] = L.OV2_EINVAL
    with pytest.raises(Ov2Error):
        _mono(t, "Begin", doepipolar=False)
    out, st, p3p, epis, poses, monos = t.trackMonoEnd()
    name, eargs = lib.calls[-1]
    assert name == "ov2_btracker_track_mono_end" and eargs[3] is not None and eargs[3][1] == NA and len(epis) == NA
    # ... and so does a refused whole call, and one of another family with another n_active
    lib.refuse = {}
    _mono(t, "Begin", doepipolar=True)
    lib.refuse ={"ov2_btracker_track_mono": L.OV2_EINVAL, "ov2_btracker_track_frame_begin": L.OV2_EINVAL}
    with pytest.raises(Ov2Error):
        _mono(t, "", doepipolar=False)
    with pytest.raises(Ov2Error):
        t.trackFrameBegin(X["imgs"][:1], X["kps"], X["pri"], None, X["n"][:1])
    out, st, p3p = t.trackFrameEnd()
    assert p3p.shape == (NA,) and lib.calls[-1][1][2] == bytes(NA * 4)


def test_a_refused_trackFrameBegin_leaves_trackFrameEnd_sized_for_the_open_step():
    t, lib = _tracker()
    t.trackFrameBegin(X["imgs"], X["kps"], X["pri"], None, X["n"])
    lib.refuse["ov2_btracker_track_frame_begin"] = L.OV2_EINVAL
    with pytest.raises(Ov2Error):
        t.trackFrameBegin(X["imgs"][:1], X["kps"], X["pri"], None, X["n"][:1])
    out, st, p3p = t.trackFrameEnd()
    assert p3p.shape == (NA,) and lib.calls[-1][1][2] == bytes(NA * 4)


ENDS = ("trackFrameEnd", "trackFramePoseEnd", "trackFrameEpiPoseEnd", "trackMonoEnd", "trackMonoResidentEnd", "createKeyframeEnd",
        "stereoKeyframeEnd", "temporalKeyframeEnd")


@pytest.mark.parametrize("end", ENDS)
def test_an_end_with_nothing_open_reaches_the_library(end):
    t, lib = _tracker()
    lib.refuse = {n: L.OV2_EINVAL for n in L.SIGNATURES if n.endswith("_end")}
    with pytest.raises(Ov2Error) as e:                                        # the library's refusal, not an AttributeError / TypeError
        getattr(t, end)()
    assert e.value.code == L.OV2_EINVAL and len(lib.calls) == 1 and lib.calls[0][0].endswith("_end")
    # ... and so does one of another kind than the open call, sized for the open call
    t.trackFrameBegin(X["imgs"], X["kps"], X["pri"], None, X["n"])
    t.createKeyframeBegin(*CASES["create_keyframe_resident"][1])              # (the stub opens whatever it is given)
    with pytest.raises(Ov2Error):
        getattr(t, end)()
    assert lib.calls[-1][0].endswith("_end")


@pytest.mark.parametrize("which, cols", [("Pose", 4), ("Epi", 8)])
def test_last_inputs_have_room_for_the_last_finished_step(which, cols):
    """the table is written for the last FINISHED step: a later refused step with fewer rows must not shrink the room"""
    t, lib = _tracker()
    stem, args, kw, _, _ = CASES["track_frame_epi_pose"]
    ep = L.EpifilterParams()
    ep.n_rows = 64
    t.trackFrameEpiPose(*args[:7], ep, *args[8:], **dict(kw, n_rows=64))
    lib.refuse["ov2_btracker_track_frame_epi_pose"] = L.OV2_EINVAL
    ep0 = L.EpifilterParams()
    with pytest.raises(Ov2Error):
        t.trackFrameEpiPose(*args[:7], ep0, *args[8:], **dict(kw, n_rows=0))
    lib.table_rows = 64
    got = getattr(t, "last%sInputs" % which)(0)
    assert np.array_equal(got[-1], 1000 + np.arange(64 * cols, dtype=np.int32).reshape(64, cols))
    lib.table_rows = {4: L.OV2_P3P_MAX_ROWS, 8: L.OV2_EPI_MAX_ROWS}[cols]     # the most the library may write
    assert getattr(t, "last%sInputs" % which)(0)[-1].shape == (lib.table_rows, cols)
