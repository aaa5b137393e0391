"""The C ABI of the loop local-map tracking (k_map_match<true> / k_map_pick, ov2slam_amd/csrc/mapmatch.hip) rejects bad arguments and
every class of malformed input without a GPU (the inputs are checked before the context is touched).  The kernels' resources are
checked in tests/test_match_resources.py."""
import ctypes as C

import numpy as np
import pytest

from tests import loopmap_ref as R


def _lib():
    import ov2slam_amd
    return ov2slam_amd.load()


def test_abi_symbols_and_wrappers_exist():
    from ov2slam_amd import _lib as L
    from ov2slam_amd import loop_closer as LC
    lib = _lib()
    assert hasattr(lib, "ov2_loop_match_to_map") and hasattr(lib, "ov2_loop_match_to_map_batch")
    assert callable(LC.loop_match_to_map) and callable(LC.loop_match_to_map_batch)
    assert (L.OV2_LOOPMAP_BEHIND, L.OV2_LOOPMAP_OUT_OF_FOV, L.OV2_LOOPMAP_OUT_OF_IMAGE, L.OV2_LOOPMAP_NO_CANDIDATE,
            L.OV2_LOOPMAP_RATIO_REJECTED, L.OV2_LOOPMAP_BEST) == (L.OV2_MATCH_BEHIND, L.OV2_MATCH_OUT_OF_FOV, L.OV2_MATCH_OUT_OF_IMAGE,
                                                                  L.OV2_MATCH_NO_CANDIDATE, L.OV2_MATCH_RATIO_REJECTED, L.OV2_MATCH_BEST)
    assert lib.ov2_version() == L.OV2_ABI_VERSION == 600


def test_null_arguments_are_einval():
    from ov2slam_amd import _lib as L
    lib = _lib()
    p, k, r = L.LoopMapParams(), L.LoopMapItem(), L.LoopMapResult()
    assert lib.ov2_loop_match_to_map(None, None, None, None) == L.OV2_EINVAL
    assert b"NULL" in lib.ov2_last_error()
    assert lib.ov2_loop_match_to_map(None, C.byref(p), None, C.byref(r)) == L.OV2_EINVAL
    assert lib.ov2_loop_match_to_map_batch(None, None, 1, C.byref(k), C.byref(r)) == L.OV2_EINVAL
    assert b"NULL" in lib.ov2_last_error()
    assert lib.ov2_loop_match_to_map_batch(None, C.byref(_params()), 1, None, None) == L.OV2_EINVAL
    assert lib.ov2_loop_match_to_map_batch(None, C.byref(_params()), -1, C.byref(k), C.byref(r)) == L.OV2_EINVAL
    assert b"n_items" in lib.ov2_last_error()


def _params(**kw):
    from ov2slam_amd import loop_closer as LC
    P = R.make_params()
    P.update(kw)
    return LC._as_loopmap_params(P)


_SCENE = []


def _scene():
    if not _SCENE:
        M = R.make_scene(R.make_params(), np.random.default_rng(3), n_kp=30, n_lm=40)
        _SCENE.append(R.flatten(M)[0])
    return dict(_SCENE[0])


def _call(item, params=None, batch=False, n_items=1):
    """the call with a NULL context: (return code, message); the result arrays must stay untouched"""
    from ov2slam_amd import loop_closer as LC
    lib = _lib()
    s, keep, n_lm, n_kp = LC._loopmap_item(item)
    r, out = LC._loopmap_result(n_lm, n_kp)
    for a in out.values():
        a.view(np.uint8)[...] = 0xEE
    p = params if params is not None else _params()
    if batch:
        rc = lib.ov2_loop_match_to_map_batch(None, C.byref(p), n_items, C.byref(s), C.byref(r))
    else:
        rc = lib.ov2_loop_match_to_map(None, C.byref(p), C.byref(s), C.byref(r))
    assert all((a.view(np.uint8) == 0xEE).all() for a in out.values()), "a rejected call wrote its outputs"
    return rc, lib.ov2_last_error()


def test_well_formed_input_reaches_the_context_check():
    """the same scene unmodified passes every input check: only the NULL context is left to object to"""
    from ov2slam_amd import _lib as L
    for batch in (False, True):
        rc, msg = _call(_scene(), batch=batch)
        assert rc == L.OV2_EINVAL and b"NULL context" in msg, msg


def _mod(item, name, fn):
    item = dict(item)
    a = np.array(item[name])
    fn(a)
    item[name] = a
    return item


def _first_row_with_two_obs(item):
    n = np.diff(item["obs_start"])
    return int(np.nonzero(n >= 2)[0][0])


MALFORMED = [
    ("kp_mp_above_table", lambda it: _mod(it, "kp_mp", lambda a: a.__setitem__(0, len(it["obs_start"]) - 1)), b"kp_mp"),
    ("kp_mp_below_minus_one", lambda it: _mod(it, "kp_mp", lambda a: a.__setitem__(0, -2)), b"kp_mp"),
    ("lm_mp_outside", lambda it: _mod(it, "lm_mp", lambda a: a.__setitem__(0, len(it["obs_start"]) - 1)), b"lm_mp"),
    ("lm_mp_negative", lambda it: _mod(it, "lm_mp", lambda a: a.__setitem__(0, -1)), b"lm_mp"),
    ("cell_kp_outside", lambda it: _mod(it, "cell_kp", lambda a: a.__setitem__(0, len(it["kp_mp"]))), b"cell_kp"),
    ("cell_kp_negative", lambda it: _mod(it, "cell_kp", lambda a: a.__setitem__(0, -1)), b"cell_kp"),
    ("obs_kfid_unsorted", lambda it: _mod(it, "obs_kfid", lambda a: a.__setitem__(it["obs_start"][_first_row_with_two_obs(it)] + 1,
                                                                                   a[it["obs_start"][_first_row_with_two_obs(it)]])), b"unsorted"),
    ("obs_start_decreases", lambda it: _mod(it, "obs_start", lambda a: a.__setitem__(1, a[2] + 1)), b"obs_start"),
    ("desc_start_decreases", lambda it: _mod(it, "desc_start", lambda a: a.__setitem__(1, a[2] + 1)), b"desc_start"),
    ("cell_start_decreases", lambda it: _mod(it, "cell_start", lambda a: a.__setitem__(1, a[-1] + 1)), b"cell_start"),
    ("obs_start_not_from_zero", lambda it: _mod(it, "obs_start", lambda a: a.__setitem__(0, -1)), b"obs_start"),
    ("cell_start_not_from_zero", lambda it: _mod(it, "cell_start", lambda a: a.__setitem__(0, 1)), b"cell_start"),
]


@pytest.mark.parametrize("batch", [False, True], ids=["single", "batch"])
@pytest.mark.parametrize("case", MALFORMED, ids=lambda c: c[0])
def test_malformed_input_is_rejected_without_a_gpu(case, batch):
    from ov2slam_amd import _lib as L
    from ov2slam_amd import loop_closer as LC
    name, make, word = case
    good = _scene()
    item = make(good)
    lib = _lib()
    # around the Python wrapper's own length checks: build the struct from the valid scene, then point it at the bad array
    s, keep, n_lm, n_kp = LC._loopmap_item(good)
    bad = {}
    for f, dt, ct in LC._LOOPMAP_FIELDS:
        if not np.array_equal(item[f], good[f]):
            bad[f] = np.ascontiguousarray(item[f], dtype=dt)
            setattr(s, f, bad[f].ctypes.data_as(C.POINTER(ct)))
    assert len(bad) == 1, (name, list(bad))
    r, out = LC._loopmap_result(n_lm, n_kp)
    for a in out.values():
        a.view(np.uint8)[...] = 0xEE
    p = _params()
    if batch:
        rc = lib.ov2_loop_match_to_map_batch(None, C.byref(p), 1, C.byref(s), C.byref(r))
    else:
        rc = lib.ov2_loop_match_to_map(None, C.byref(p), C.byref(s), C.byref(r))
    msg = lib.ov2_last_error()
    assert rc == L.OV2_EINVAL and word in msg and b"NULL context" not in msg, (name, rc, msg)
    assert all((a.view(np.uint8) == 0xEE).all() for a in out.values()), "a rejected call wrote its outputs"


@pytest.mark.parametrize("batch", [False, True], ids=["single", "batch"])
def test_negative_counts_and_null_arrays(batch):
    from ov2slam_amd import _lib as L
    from ov2slam_amd import loop_closer as LC
    lib = _lib()
    item = _scene()

    def call(s, r):
        if batch:
            return lib.ov2_loop_match_to_map_batch(None, C.byref(_params()), 1, C.byref(s), C.byref(r))
        return lib.ov2_loop_match_to_map(None, C.byref(_params()), C.byref(s), C.byref(r))
    for field in ("n_kp", "n_mp", "n_lm"):
        s, keep, n_lm, n_kp = LC._loopmap_item(item)
        setattr(s, field, -1)
        r, out = LC._loopmap_result(n_lm, n_kp)
        assert call(s, r) == L.OV2_EINVAL
        assert b"negative count" in lib.ov2_last_error()
    for field in ("Tcw", "kp_px", "kp_mp", "kp_matched", "cell_start", "cell_kp", "obs_start", "obs_kfid", "desc_start", "desc", "lm_mp", "lm_wpt"):
        s, keep, n_lm, n_kp = LC._loopmap_item(item)
        setattr(s, field, None)
        r, out = LC._loopmap_result(n_lm, n_kp)
        assert call(s, r) == L.OV2_EINVAL, field
        assert b"NULL" in lib.ov2_last_error() and b"NULL context" not in lib.ov2_last_error(), field
    for field in ("lm_status", "lm_kp", "lm_dist", "lm_projpx", "kp_lm", "kp_dist"):
        s, keep, n_lm, n_kp = LC._loopmap_item(item)
        r, out = LC._loopmap_result(n_lm, n_kp)
        setattr(r, field, None)
        assert call(s, r) == L.OV2_EINVAL, field
        assert b"result buffer" in lib.ov2_last_error(), field


def test_unsupported_parameters():
    from ov2slam_amd import _lib as L
    item = _scene()
    for kw in (dict(D=(0.1, 0.01, 0.001)), dict(D=(0.1,) * 6), dict(D=(0.1,) * 14), dict(D=(0.1,) * 5, model="fisheye"),
               dict(desc_bytes=64), dict(desc_bytes=16)):
        rc, msg = _call(item, params=_params(**kw))
        assert rc == L.OV2_EUNSUPPORTED and msg, (kw, msg)
    rc, msg = _call(item, batch=True, n_items=65536)
    assert rc == L.OV2_EUNSUPPORTED and b"65535" in msg
    for kw in (dict(ncellsize=0), dict(img_w=0), dict(img_h=-480)):
        rc, msg = _call(item, params=_params(**kw))
        assert rc == L.OV2_EINVAL and b"not positive" in msg, (kw, msg)
    p = _params()
    p.model = 7
    rc, msg = _call(item, params=p)
    assert rc == L.OV2_EINVAL and b"camera model" in msg
