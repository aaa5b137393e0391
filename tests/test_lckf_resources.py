"""The kernels of the loop closer's keyframe preparation (ov2slam_amd/csrc/lckf.hip): a device-only compile for gfx950 shows no scratch
and at most 128 VGPRs (four wavefronts per SIMD) for every one of them; the C ABI rejects bad arguments and every class of malformed
input without a GPU (the inputs are checked before the context is touched) and writes none of its outputs then; the Python wrapper
checks shapes; and the tile constants, which the GPU test sizes are built around, are the ones the source declares."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "ov2slam_amd", "csrc", "lckf.hip")
LCKF_TILE_W = 64           # output pixels of one work-group of k_lckf_fast
LCKF_TILE_H = 16
LCKF_HALO = 4              # 3 for the ring, 1 for the neighbours' scores
KERNELS = ("k_lckf_paint", "k_lckf_fast", "k_lckf_cut", "k_lckf_rows", "k_lckf_scan", "k_lckf_emit")


def test_tile_constants_are_those_of_the_kernel():
    txt = open(SRC).read()
    got = {k: int(v) for k, v in re.findall(r"^constexpr int (LCKF_\w+) = (\d+);", txt, re.M)}
    assert got["LCKF_TILE_W"] == LCKF_TILE_W and got["LCKF_TILE_H"] == LCKF_TILE_H and got["LCKF_HALO"] == LCKF_HALO, got


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_kernels_use_no_scratch_and_128_vgprs(tmp_path):
    out = str(tmp_path / "lckf.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                    "--cuda-device-only", "-S", SRC, "-o", out], check=True, capture_output=True)
    txt = open(out).read()
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        res[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)\s", m.group(2))}
    names = [n for n in res if "k_lckf" in n]
    assert len(names) == len(KERNELS) and all(any(k in n for n in names) for k in KERNELS), names
    for n in names:
        assert res[n]["private_segment_fixed_size"] == 0, (n, res[n])
        assert res[n]["next_free_vgpr"] <= 128, (n, res[n])
    # k_lckf_fast: the pixel tile with its halo, the score tile with one pixel around it (pitch padded to words), the output tile
    fast = [n for n in names if "k_lckf_fast" in n][0]
    pix = (LCKF_TILE_W + 2 * LCKF_HALO) * (LCKF_TILE_H + 2 * LCKF_HALO)
    sc = (LCKF_TILE_W + 4) * (LCKF_TILE_H + 2)
    lds = sum((b + 15) // 16 * 16 for b in (pix, sc, LCKF_TILE_W * LCKF_TILE_H))
    assert res[fast]["group_segment_fixed_size"] == lds == 3984, (res[fast], lds)


def _lib():
    import ov2slam_amd
    return ov2slam_amd.load()


def _img(w=80, h=60):
    return np.random.default_rng(1).integers(0, 256, (h, w), dtype=np.uint8)


def _call(edit=None, params=None, w=80, h=60, stride=None, n_excl=5, img_null=False, excl_null=False, result_null=False, kept_cap=16, all_cap=16):
    """ov2_lckf_prepare with a NULL context: (return code, message); asserts that no output byte was written"""
    from ov2slam_amd import loop_closer as LC
    lib = _lib()
    img = _img(max(w, 1), max(h, 1))
    e = np.random.default_rng(2).uniform(0, 50, (max(n_excl, 1), 2)).astype(np.float32)
    r, out = LC.lckf_buffers(kept_cap, all_cap, fill=0xEE)
    r.n_all = r.cut = r.n_kept = r.n_desc = -77
    p = params if params is not None else LC.lckf_params()
    if edit:
        edit(r)
    rc = lib.ov2_lckf_prepare(None, None if img_null else img.ctypes.data_as(C.c_void_p), w, h, img.strides[0] if stride is None else stride,
                              C.byref(p) if p is not False else None, None if excl_null else e.ctypes.data_as(C.c_void_p), n_excl,
                              None if result_null else C.byref(r))
    assert all((a.view(np.uint8) == 0xEE).all() for a in out.values()), "a rejected call wrote its outputs"
    assert (r.n_all, r.cut, r.n_kept, r.n_desc) == (-77,) * 4, "a rejected call wrote its counts"
    return rc, lib.ov2_last_error()


def test_well_formed_input_reaches_the_context_check():
    from ov2slam_amd import _lib as L
    from ov2slam_amd import loop_closer as LC
    for kw in (dict(), dict(n_excl=0, excl_null=True), dict(kept_cap=0, all_cap=0), dict(w=6, h=9), dict(w=1, h=1), dict(w=32767, h=1, stride=32767),
               dict(params=LC.lckf_params(threshold=-5, retain=-1, excl_radius=0)), dict(params=LC.lckf_params(threshold=999, retain=0, excl_radius=64)),
               dict(edit=lambda r: (setattr(r, "all_xy", None), setattr(r, "all_resp", None), setattr(r, "all_cap", 0)))):
        rc, msg = _call(**kw)
        assert rc == L.OV2_EINVAL and b"NULL context" in msg, (kw, msg)


def _set(**kw):
    def edit(r):
        for k, v in kw.items():
            setattr(r, k, v)
    return edit


MALFORMED = [
    ("params_null", dict(params=False), b"NULL params"),
    ("image_null", dict(img_null=True), b"NULL image"),
    ("result_null", dict(result_null=True), b"NULL image / result"),
    ("n_excl_negative", dict(n_excl=-1), b"negative count"),
    ("excl_null", dict(excl_null=True), b"excl_xy == NULL"),
    ("width_zero", dict(w=0), b"image size"),
    ("height_negative", dict(h=-3), b"image size"),
    ("stride_below_width", dict(stride=79), b"stride < width"),
    ("stride_negative", dict(stride=-80), b"stride < width"),
    ("radius_negative", dict(params=(20, 300, -1)), b"excl_radius"),
    ("radius_65", dict(params=(20, 300, 65)), b"excl_radius"),
    ("kept_cap_negative", dict(edit=_set(kept_cap=-1)), b"negative capacity"),
    ("all_cap_negative", dict(edit=_set(all_cap=-1)), b"negative capacity"),
    ("kept_xy_null", dict(edit=_set(kept_xy=None)), b"result buffer"),
    ("kept_resp_null", dict(edit=_set(kept_resp=None)), b"result buffer"),
    ("kept_valid_null", dict(edit=_set(kept_valid=None)), b"result buffer"),
    ("kept_desc_null", dict(edit=_set(kept_desc=None)), b"result buffer"),
    ("all_xy_null", dict(edit=_set(all_xy=None)), b"result buffer"),
    ("all_resp_null", dict(edit=_set(all_resp=None)), b"result buffer"),
]


@pytest.mark.parametrize("case", MALFORMED, ids=lambda c: c[0])
def test_malformed_input_is_rejected_without_a_gpu(case):
    from ov2slam_amd import _lib as L
    from ov2slam_amd import loop_closer as LC
    name, kw, word = case
    kw = dict(kw)
    if isinstance(kw.get("params"), tuple):
        kw["params"] = LC.lckf_params(*kw["params"])
    rc, msg = _call(**kw)
    assert rc == L.OV2_EINVAL and word in msg and b"NULL context" not in msg, (name, rc, msg)


def test_unsupported_sizes():
    from ov2slam_amd import _lib as L
    for kw in (dict(w=32768, h=1, stride=32768), dict(w=4, h=32768), dict(w=1 << 20, h=2, stride=1 << 20)):
        rc, msg = _call(**kw)
        assert rc == L.OV2_EUNSUPPORTED and b"2^15" in msg, (kw, msg)


def test_other_entry_points_check_their_inputs_first():
    from ov2slam_amd import _lib as L
    from ov2slam_amd import loop_closer as LC
    lib = _lib()
    p = LC.lckf_params()
    r, out = LC.lckf_buffers(4, 0, fill=0xEE)
    assert lib.ov2_lckf_params_init(None) == L.OV2_EINVAL
    q = L.LckfParams()
    assert lib.ov2_lckf_params_init(C.byref(q)) == L.OV2_OK and (q.threshold, q.retain, q.excl_radius) == (20, 300, 2)
    assert lib.ov2_tracker_lckf_prepare(None, C.byref(p), None, 0, C.byref(r)) == L.OV2_EINVAL and b"NULL tracker" in lib.ov2_last_error()
    assert lib.ov2_btracker_lckf_prepare(None, 1, C.byref(p), None, None, 0, None) == L.OV2_EINVAL and b"NULL" in lib.ov2_last_error()
    one = 1                                             # any non-NULL address: nothing is dereferenced before the checks fail
    bd = lambda **kw: lib.ov2_lckf_prepare_batch_d(*[kw.get(k, v) for k, v in (
        ("ctx", None), ("params", C.byref(p)), ("img", one), ("w", 80), ("h", 60), ("pitch", 80), ("item_stride", 4800), ("n_items", 2),
        ("excl", one), ("excl_cap", 4), ("n_excl", one), ("all_xy", None), ("all_resp", None), ("all_cap", 0), ("kept_xy", one),
        ("kept_resp", one), ("kept_valid", one), ("kept_desc", one), ("kept_cap", 8), ("counts", one))])
    assert bd() == L.OV2_EINVAL and b"NULL context" in lib.ov2_last_error()
    assert bd(n_items=0, img=None, counts=None) == L.OV2_EINVAL and b"NULL context" in lib.ov2_last_error()
    for kw, code, word in ((dict(params=None), L.OV2_EINVAL, b"NULL params"), (dict(n_items=-1), L.OV2_EINVAL, b"n_items"),
                           (dict(n_items=65536), L.OV2_EUNSUPPORTED, b"65535"), (dict(pitch=79), L.OV2_EINVAL, b"stride < width"),
                           (dict(item_stride=4799), L.OV2_EINVAL, b"item_stride"), (dict(w=40000, pitch=40000), L.OV2_EUNSUPPORTED, b"2^15"),
                           (dict(img=None), L.OV2_EINVAL, b"NULL device buffer"), (dict(counts=None), L.OV2_EINVAL, b"NULL device buffer"),
                           (dict(n_excl=None), L.OV2_EINVAL, b"NULL device buffer"), (dict(kept_desc=None), L.OV2_EINVAL, b"NULL device buffer"),
                           (dict(all_cap=4), L.OV2_EINVAL, b"NULL device buffer"), (dict(excl_cap=-1), L.OV2_EINVAL, b"negative capacity"),
                           (dict(kept_cap=-2), L.OV2_EINVAL, b"negative capacity")):
        assert bd(**kw) == code and word in lib.ov2_last_error() and b"NULL context" not in lib.ov2_last_error(), (kw, lib.ov2_last_error())
    assert all((a.view(np.uint8) == 0xEE).all() for a in out.values())


def test_python_wrapper_checks_shapes():
    from ov2slam_amd import loop_closer as LC
    p = LC.lckf_params()
    assert (p.threshold, p.retain, p.excl_radius) == (20, 300, 2)
    assert LC.lckf_params(retain=-1, excl_radius=5).retain == -1
    with pytest.raises(ValueError):
        LC._excl(np.zeros((3, 3), np.float32))
    with pytest.raises(ValueError):
        LC._excl(np.zeros(5, np.float32))
    assert LC._excl(None).shape == (0, 2) and LC._excl([]).shape == (0, 2) and LC._excl([(1, 2)]).dtype == np.float32
    with pytest.raises(ValueError):
        LC._image(np.zeros((4, 5), np.float32))
    with pytest.raises(ValueError):
        LC._image(np.zeros((4, 5, 3), np.uint8))
    with pytest.raises(ValueError):
        LC._image(np.zeros((0, 5), np.uint8))
    strided = np.zeros((8, 20), np.uint8)[:, :12]
    assert LC._image(strided).strides == (20, 1)                               # a row stride is passed on, not copied away
    assert LC._image(np.zeros((8, 20), np.uint8)[:, ::2]).strides == (10, 1)
    with pytest.raises(ValueError):
        LC.lckf_buffers(-1, 0)
    with pytest.raises(ValueError):
        LC.lckf_prepare_batch(None, p, np.zeros((2, 8, 8), np.uint8), [None])
