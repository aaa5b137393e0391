"""Scope row f23 without a GPU (tests/temporalkf_ref.py): over the scripted run of six keyframes the anchor-table rule (b) selects, for
every keypoint of every call, the source keyframe, src_unpx, src_bv and source pose that the map model (a) selects by the reference's
own rule; and the script makes tests/tri_ref.py take every branch the GPU test relies on.  Nothing is skipped: the scene is chosen so
that the reference alone meets every condition."""
import numpy as np
import pytest

from tests import temporalkf_ref as R

NAME = "mono-pinhole"
ITEMS = (0, 1, 2, 3)


@pytest.fixture(scope="module")
def logs():
    return {(b, stereo): R.simulate(NAME, b, stereo=stereo) for b in ITEMS for stereo in (False, True)}


def test_the_script_has_its_events(logs):
    log = logs[(0, False)]
    assert [e["tag"] for e in log] == ["kf0", "kf1", "kf1_again", "kf2", "kf3", "kf4", "kf5"] and R.N_KF >= 6
    S = R.script(NAME)
    for b in ITEMS[:3]:
        ids = [set(int(l) for l in f["lmid"]) for f in S["items"][b]["frames"]]
        assert all(ids[k + 1] - ids[k] for k in range(R.N_KF - 1)), "births at every keyframe"
        assert all(ids[k] - ids[k + 1] for k in range(R.N_KF - 1)), "deaths at every keyframe"
        assert all(len(i) <= R.N_MAX for i in ids)
    # item 3 carries the sizes
    assert [len(f["lmid"]) for f in S["items"][3]["frames"][:2]] == [0, 1]
    assert len(S["items"][3]["frames"][2]["lmid"]) >= 2 and set(S["items"][3]["frames"][2]["kind"]) == {"init3d"}


@pytest.mark.parametrize("stereo", [False, True])
@pytest.mark.parametrize("b", ITEMS)
def test_the_table_selects_what_the_map_selects(logs, b, stereo):
    """(b) against (a) at every call: the same candidates, the same source keyframe, the same source keypoint and pose"""
    for e in logs[(b, stereo)]:
        assert e["a"] == e["b"], (e["tag"], sorted(set(e["a"].items()) ^ set(e["b"].items())))
        assert e["same_src"], e["tag"]
        assert e["rows"] == sorted(set(e["rows"])) and set(e["a"].values()) <= set(e["rows"])
        assert len(e["rows"]) <= R.N_SRC_MAX
    total = sum(len(e["a"]) for e in logs[(b, stereo)])
    assert total > 0 or b == 3


def test_the_script_takes_every_branch(logs):
    """each population is non-empty in at least one item, on tri_ref alone"""
    some = lambda pred, stereo=False: any(pred(e, lm, st) for b in ITEMS for e in logs[(b, stereo)] for lm, st in e["status"].items())
    why = lambda e, lm: e["reason"].get(lm, (None, 0.0))
    assert some(lambda e, lm, st: st & R.OK)
    assert some(lambda e, lm, st: (st & R.REMOVE_OBS) and why(e, lm)[0] == "depth" and why(e, lm)[1] > 20.0)
    assert some(lambda e, lm, st: (st & R.TRIED) and not (st & (R.OK | R.REMOVE_OBS)) and why(e, lm)[0] == "depth" and why(e, lm)[1] <= 20.0)
    assert some(lambda e, lm, st: (st & R.TRIED) and not (st & R.OK) and why(e, lm)[0] == "reproj")
    assert some(lambda e, lm, st: st & R.NO_MOTION, stereo=True) and not some(lambda e, lm, st: st & R.NO_MOTION, stereo=False)
    # REMOVE_OBS is exactly "rejected with more than 20 px of parallax"
    for key, log in logs.items():
        for e in log:
            for lm, st in e["status"].items():
                if (st & R.TRIED) and not (st & R.OK):
                    assert bool(st & R.REMOVE_OBS) == (e["reason"][lm][1] > 20.0), (key, e["tag"], lm)
    for b in ITEMS[:3]:
        log = logs[(b, False)]
        by = {e["tag"]: e for e in log}
        # anchors at this keyframe, slots that are 3-D already, anchors at three keyframes or more
        for e in log[1:]:
            assert any(k == e["rows"][-1] for k in e["anchors"].values()), (b, e["tag"])
            assert e["n_3d"] > 0 or e["tag"] == "kf1"                     # from the second call on: the points keyframe 1 made
        assert max(len(set(e["a"].values())) for e in log) >= 3, b
        # a REMOVE_OBS at one keyframe, a successful triangulation of the same point at the next
        gone1 = {lm for lm, st in by["kf1"]["status"].items() if st & R.REMOVE_OBS}
        assert gone1 and any(by["kf2"]["status"].get(lm, 0) & R.OK for lm in gone1), b
        # the second call on keyframe 1: those slots are in the frame and no longer in the keyframe; nothing new happens
        again = by["kf1_again"]
        assert again["n_not_in_kf"] == len(gone1) and by["kf1"]["n_not_in_kf"] == 0
        assert not any(st & (R.OK | R.REMOVE_OBS) for st in again["status"].values())
        assert again["rows"] == by["kf1"]["rows"] and again["anchors"] == by["kf1"]["anchors"]
        # the culled keyframe is nobody's anchor afterwards; before, it was somebody's
        k1 = R.kfid_of(1, b)
        assert k1 in by["kf3"]["rows"] and k1 not in by["kf4"]["rows"] and k1 not in by["kf5"]["rows"]
        assert all(v != k1 for v in by["kf4"]["a"].values())
    # the sizes of item 3: nothing to do with no slot, with one fresh slot and with every slot 3-D
    l3 = {e["tag"]: e for e in logs[(3, False)]}
    assert l3["kf0"]["status"] == {} and list(l3["kf1"]["status"].values()) == [0] and set(l3["kf2"]["status"].values()) == {0}
    assert l3["kf2"]["n_3d"] == len(l3["kf2"]["status"]) >= 2


def test_a_moved_pose_moves_the_points():
    """the BA change before keyframe 2 reaches the points anchored at keyframe 0: with and without it they differ"""
    S = R.script(NAME)
    item = S["items"][0]
    with_ba = {e["tag"]: e for e in R.simulate(NAME, 0)}
    assert R.kfid_of(0, 0) in with_ba["kf2"]["a"].values()
    t = R.AnchorTable([1], [5], [[1.0, 2.0]], [[0.0, 0.0, 1.0]], [5], [item["poses"][0]])
    assert t.set_poses([(5, item["poses"][1]), (6, item["poses"][1])]) == 1 and np.array_equal(t.row_Twc[0], item["poses"][1])


def test_the_table_overflows_at_n_src_max():
    """births at three keyframes in a row need three rows: with two the third keyframe overflows and the table stays"""
    S = R.script(NAME)
    item = S["items"][0]
    tb = R.AnchorTable()
    seen = []
    for k in range(3):
        kf = R.keyframe_of(S, R.frame_for(item, k, {}), R.kfid_of(k, 0), item["poses"][k])
        nt = tb.advance(kf["id"], kf["Twc"], kf["lmid"], kf["unpx"], kf["bv"], 2)
        seen.append(nt is None)
        tb = tb if nt is None else nt
    assert seen == [False, False, True] and [int(v) for v in tb.row_kfid] == [R.kfid_of(0, 0), R.kfid_of(1, 0)]
