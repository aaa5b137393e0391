"""k_knn / k_knn_merge (ov2slam_amd/csrc/knn.hip): a device-only compile for gfx950 shows no scratch and at most 128 VGPRs (four wavefronts per
SIMD); the C ABI of the descriptor matching rejects bad arguments and every class of malformed input without a GPU (the inputs are
checked before the context is touched) and writes none of its outputs then; and the kernel's tiling constants, which the GPU test
sizes are built around, are the ones the source declares."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import knn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "ov2slam_amd", "csrc", "knn.hip")
KNN_QUERIES = 256          # query rows per work-group
KNN_TILE = 256             # train rows per LDS tile
KNN_FILL = 256             # a call of q_tiles * n_items work-groups splits its train tiles over grid.z in min(tiles, KNN_FILL // work-groups) ranges


def test_tiling_constants_are_those_of_the_kernel():
    txt = open(SRC).read()
    got = {k: int(v) for k, v in re.findall(r"^constexpr int (KNN_\w+) = (\d+);", txt, re.M)}
    assert got["KNN_QUERIES"] == KNN_QUERIES and got["KNN_TILE"] == KNN_TILE and got["KNN_FILL"] == KNN_FILL, got


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_k_knn_kernels_use_no_scratch_and_128_vgprs(tmp_path):
    out = str(tmp_path / "knn.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                    "--cuda-device-only", "-S", SRC, "-o", out], check=True, capture_output=True)
    txt = open(out).read()
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        res[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)\s", m.group(2))}
    names = [n for n in res if "k_knn" in n]
    assert len(names) == 2, names                                       # k_knn, k_knn_merge
    for n in names:
        assert res[n]["private_segment_fixed_size"] == 0, (n, res[n])
        assert res[n]["next_free_vgpr"] <= 128, (n, res[n])
        assert res[n]["group_segment_fixed_size"] == (0 if "merge" in n else 32 * KNN_TILE), (n, res[n])


def _lib():
    import ov2slam_amd
    return ov2slam_amd.load()


def _case(n_q=40, n_t=50):
    return R.make_case(np.random.default_rng(3), n_q, n_t)


def _call(query, train, params=None, batch=False, n_items=1, edit=None):
    """the call with a NULL context: (return code, message); asserts that no output byte was written"""
    from ov2slam_amd import loop_closer as LC
    lib = _lib()
    s, keep = LC._item(query, train)
    r, out = LC._result(max(s.n_query, 1))
    for a in out.values():
        a.view(np.uint8)[...] = 0xEE
    p = params if params is not None else LC.knn_params()
    if edit:
        edit(s, r)
    if batch:
        rc = lib.ov2_knn_match_batch(None, C.byref(p), n_items, C.byref(s), C.byref(r))
    else:
        rc = lib.ov2_knn_match(None, C.byref(p), C.byref(s), C.byref(r))
    assert all((a.view(np.uint8) == 0xEE).all() for a in out.values()), "a rejected call wrote its outputs"
    return rc, lib.ov2_last_error()


def test_null_arguments_are_einval():
    from ov2slam_amd import _lib as L
    from ov2slam_amd import loop_closer as LC
    lib = _lib()
    p, k, r = LC.knn_params(), L.KnnItem(), L.KnnResult()
    assert lib.ov2_knn_match(None, None, None, None) == L.OV2_EINVAL
    assert b"NULL" in lib.ov2_last_error()
    assert lib.ov2_knn_match(None, C.byref(p), None, C.byref(r)) == L.OV2_EINVAL
    assert lib.ov2_knn_match(None, C.byref(p), C.byref(k), None) == L.OV2_EINVAL
    assert lib.ov2_knn_match(None, None, C.byref(k), C.byref(r)) == L.OV2_EINVAL
    assert b"NULL params" in lib.ov2_last_error()
    assert lib.ov2_knn_match_batch(None, None, 1, C.byref(k), C.byref(r)) == L.OV2_EINVAL
    assert lib.ov2_knn_match_batch(None, C.byref(p), 1, None, None) == L.OV2_EINVAL
    assert b"NULL" in lib.ov2_last_error() and b"NULL context" not in lib.ov2_last_error()
    assert lib.ov2_knn_match_batch(None, C.byref(p), -1, C.byref(k), C.byref(r)) == L.OV2_EINVAL
    assert b"n_items" in lib.ov2_last_error()


@pytest.mark.parametrize("batch", [False, True], ids=["single", "batch"])
def test_well_formed_input_reaches_the_context_check(batch):
    """the same case unmodified passes every input check: only the NULL context is left to object to"""
    from ov2slam_amd import _lib as L
    q, t = _case()
    for qq, tt in ((q, t), (q[:0], t), (q, t[:0]), (q, t[:1])):
        rc, msg = _call(qq, tt, batch=batch)
        assert rc == L.OV2_EINVAL and b"NULL context" in msg, msg
    lib = _lib()
    from ov2slam_amd import loop_closer as LC
    assert lib.ov2_knn_match_batch(None, C.byref(LC.knn_params()), 0, None, None) == L.OV2_EINVAL
    assert b"NULL context" in lib.ov2_last_error()


def _set(**kw):
    def edit(s, r):
        for k, v in kw.items():
            setattr(s if hasattr(s, k) else r, k, v)
    return edit


MALFORMED = [
    ("n_query_negative", _set(n_query=-1), b"negative count"),
    ("n_train_negative", _set(n_train=-1), b"negative count"),
    ("query_null", _set(query=None), b"query == NULL"),
    ("train_null", _set(train=None), b"train == NULL"),
    ("idx_null", _set(idx=None), b"result buffer"),
    ("dist_null", _set(dist=None), b"result buffer"),
    ("good_null", _set(good=None), b"result buffer"),
    ("pair_query_null", _set(pair_query=None), b"result buffer"),
    ("pair_train_null", _set(pair_train=None), b"result buffer"),
]


@pytest.mark.parametrize("batch", [False, True], ids=["single", "batch"])
@pytest.mark.parametrize("case", MALFORMED, ids=lambda c: c[0])
def test_malformed_input_is_rejected_without_a_gpu(case, batch):
    from ov2slam_amd import _lib as L
    name, edit, word = case
    q, t = _case()
    rc, msg = _call(q, t, batch=batch, edit=edit)
    assert rc == L.OV2_EINVAL and word in msg and b"NULL context" not in msg, (name, rc, msg)


@pytest.mark.parametrize("batch", [False, True], ids=["single", "batch"])
def test_bad_parameters(batch):
    from ov2slam_amd import _lib as L
    from ov2slam_amd import loop_closer as LC
    q, t = _case()
    for kw, word in ((dict(max_dist=-1), b"max_dist"), (dict(ratio=-0.1), b"ratio"), (dict(ratio=float("nan")), b"ratio"),
                     (dict(ratio=float("inf")), b"ratio"), (dict(ratio=float("-inf")), b"ratio")):
        rc, msg = _call(q, t, params=LC.knn_params(**kw), batch=batch)
        assert rc == L.OV2_EINVAL and word in msg and b"NULL context" not in msg, (kw, msg)
    for kw in (dict(max_dist=0), dict(ratio=0.0), dict(max_dist=256, ratio=1.0), dict(max_dist=1000, ratio=7.5)):
        rc, msg = _call(q, t, params=LC.knn_params(**kw), batch=batch)
        assert rc == L.OV2_EINVAL and b"NULL context" in msg, (kw, msg)


def test_unsupported_sizes():
    from ov2slam_amd import _lib as L
    from ov2slam_amd import loop_closer as LC
    q, t = _case()
    for nb in (16, 31, 33, 64, 0, -32):
        for batch in (False, True):
            rc, msg = _call(q, t, params=LC.knn_params(desc_bytes=nb, max_dist=128), batch=batch)
            assert rc == L.OV2_EUNSUPPORTED and b"32 bytes" in msg, (nb, msg)
    rc, msg = _call(q, t, batch=True, n_items=65536)
    assert rc == L.OV2_EUNSUPPORTED and b"65535" in msg


def test_python_wrapper_checks_shapes():
    from ov2slam_amd import loop_closer as LC
    with pytest.raises(ValueError):
        LC._item(np.zeros((3, 16), np.uint8), np.zeros((3, 32), np.uint8))
    with pytest.raises(ValueError):
        LC._item(np.zeros((3, 32), np.uint8), np.zeros(64, np.uint8))
    p = LC.knn_params()
    assert (p.desc_bytes, p.max_dist, p.ratio) == (32, 128, 0.85)
    assert LC.knn_params(max_dist=96, ratio=0.7).max_dist == 96
