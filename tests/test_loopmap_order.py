"""loopLocalMapReferenceOrder (ov2slam_amd/host/loop_closer.hpp), the set-building walk of LoopCloser::trackLoopLocalMap with literal
std::unordered_set inserts and erases, without a GPU: tests/cpp/loopmap_order_check.cpp holds it against a literal transcription of
src/loop_closer.cpp:505-562 (same pairs, same local map in the same iteration order), also built as a stand-alone program with the
address and undefined-behaviour sanitizers, and what it returns is the set, the pairs and the vmatchedkpids of the numpy replay
(tests/loopmap_ref.py)."""
import os
import subprocess

import numpy as np
import pytest

from tests import loopmap_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _crafted_walks():
    """(lckf, {kfid: (in_map, [lmid ...])}, observed, vkplmids)"""
    walks = []
    # the +-15 window: `continue` below, `break` above
    walks.append((100, {84: (1, [1]), 85: (1, [2]), 100: (1, [3]), 115: (1, [4]), 116: (1, [5]), 130: (1, [6])}, [], []))
    # a keyframe the map no longer holds; the loop keyframe is not in its own covisibility map
    walks.append((100, {98: (1, [1, 2]), 99: (0, [50, 51])}, [], []))
    walks.append((100, {98: (1, [1, 2]), 99: (0, []), 100: (1, [7, 8])}, [], []))
    # observed points are paired once; an existing (lmid, lmid) pair is not doubled; paired points leave the local set
    walks.append((100, {99: (1, [1, 2, 3, 2]), 100: (1, [3, 4, 5, 1])}, [2, 4, 9], [(4, 4), (9, 5)]))
    # nothing at all, and the loop keyframe alone
    walks.append((7, {}, [], [(1, 2)]))
    walks.append((7, {7: (1, list(range(1000, 1400, 3)))}, [1003, 1300], [(5, 1006), (1003, 1003)]))
    # a few thousand ids over several keyframes: the set rehashes many times
    rng = np.random.default_rng(5)
    cov = {int(k): (1, [int(v) for v in rng.integers(0, 6000, 700)]) for k in range(186, 217, 3)}
    walks.append((200, cov, [int(v) for v in rng.integers(0, 6000, 300)], [(int(a), int(b)) for a, b in rng.integers(0, 6000, (120, 2))]))
    return walks


def _scene_walks():
    walks = []
    for seed in range(3):
        M = R.make_scene(R.make_params(), np.random.default_rng(40 + seed))
        lc = M["lckf"]["kfid_"]
        cov = {k: (1 if k in M["cokfs"] else 0, M["cokfs"].get(k, [])) for k in set(M["lckf"]["cov"]) | set(M["cokfs"])}
        walks.append((lc, cov, list(M["newkf"]["mapkps_"]), list(M["vkplmids"])))
    return walks


def _as_map(walk):
    """the walk as a toy map of tests/loopmap_ref.py (every point behind the camera: only the walk matters)"""
    lc, cov, observed, vk = walk
    cokfs = {k: ids for k, (present, ids) in cov.items() if present}
    mps = {i: dict(is3d_=True, wpt=np.array([0.0, 0.0, -1.0]), set_kfids_=[1], map_kf_desc_={1: np.zeros(32, np.uint8)})
           for ids in cokfs.values() for i in ids}
    nbw, nbh = R.grid_width(R.make_params())
    return dict(params=R.make_params(), newkf=dict(kfid_=500, mapkps_={i: (np.float32(10), np.float32(10)) for i in observed},
                                                   vgridkps_=[[] for _ in range(nbw * nbh)]),
                Tcw=np.array([0, 0, 0, 0, 0, 0, 1.0]), lckf=dict(kfid_=lc, cov={k: 10 for k in cov}), cokfs=cokfs, mps=mps,
                vkplmids=list(vk), local_order=None)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_reference_order_helper_against_the_literal_walk(tmp_path, sanitize):
    exe = tmp_path / "loopmap_order_check"
    flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags +
                          [os.path.join(ROOT, "tests", "cpp", "loopmap_order_check.cpp"), "-o", str(exe)])
    walks = _crafted_walks() + _scene_walks()
    words = [len(walks)]
    for lc, cov, observed, vk in walks:
        words += [lc, len(cov)]
        for k in sorted(cov, reverse=True):                             # any order: the program sorts by keyframe id as std::map does
            words += [k, cov[k][0], len(cov[k][1])] + list(cov[k][1])
        words += [len(observed)] + list(observed) + [len(vk)] + [v for p in vk for v in p]
    src, dst = tmp_path / "walks.bin", tmp_path / "out.bin"
    np.asarray(words, np.int32).tofile(src)
    r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    raw = np.fromfile(dst, np.int32)
    o = 0
    for w, walk in enumerate(walks):
        parts = []
        for _ in range(3):
            n = int(raw[o]); parts.append([int(v) for v in raw[o + 1:o + 1 + n]]); o += 1 + n
        order, pairs, matched = parts
        vk, info = R.replay(_as_map(walk))
        assert sorted(order) == sorted(info["local"]) and len(set(order)) == len(order), w
        assert list(zip(pairs[0::2], pairs[1::2])) == info["walk_vkplmids"], w
        assert matched == [k for k, _ in info["walk_vkplmids"]], w
    assert o == len(raw)
    # the crafted walks' literals
    assert sorted(R.replay(_as_map(walks[0]))[1]["local"]) == [2, 3, 4]
    assert sorted(R.replay(_as_map(walks[1]))[1]["local"]) == [1, 2]
    assert R.replay(_as_map(walks[3]))[1]["walk_vkplmids"] == [(4, 4), (9, 5), (2, 2)]
