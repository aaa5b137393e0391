"""ov2_btracker_stereo_keyframe (scope row f22) without a GPU: the slot-order cell table of tests/stereokf_ref.py on hand-written
frames, and the conditions of the scenario tests/test_gpu_stereokf.py plays -- every config's frames make the block take every branch
the geometry can produce.  One branch cannot be produced: under rectification the depth gate (left.z < 0.1 m) would need a disparity
above fx * baseline / 0.1 = 252 px, two thirds of the 376 px image, where the scene's is 12; test_rectified_depth_gate_is_out_of_reach states the arithmetic."""
import numpy as np
import pytest

from tests import priors_ref as PR
from tests import stereokf_ref as R


def _table(px, w=100, h=70, cell=35):
    cs, ck = R.cell_tables(np.array(px, np.float32).reshape(-1, 2), w, h, cell)
    return cs.tolist(), ck.tolist()


def test_cell_table_in_slot_order():
    # 100 x 70 px, cells of 35: a grid of 3 x 2.  Slots 0, 2, 5 share cell 0 and stand in that order whatever their positions
    px = [(30.0, 30.0), (40.0, 10.0), (1.0, 34.9), (80.0, 60.0), (99.0, 0.0), (20.0, 3.0)]
    cs, ck = _table(px)
    assert cs == [0, 3, 4, 5, 5, 5, 6] and ck == [0, 2, 5, 1, 4, 3]
    assert cs[3] == cs[4] == cs[5]                                       # cells 3 and 4 are empty
    # a keypoint exactly on a cell border belongs to the cell that starts there, in x and in y
    cs, ck = _table([(35.0, 0.0), (34.999, 0.0), (0.0, 35.0), (70.0, 69.0)])
    assert cs == [0, 1, 2, 2, 3, 3, 4] and ck == [1, 0, 2, 3]
    # outside the image: left of it, below it, right of the grid's last column, beyond its last row, not a number: in no cell.  The
    # grid reaches past the image (3 x 35 = 105 > 100): a keypoint at x = 104 still has a cell, one at 105 has none
    cs, ck = _table([(-0.5, 10.0), (10.0, -1.0), (105.0, 10.0), (10.0, 70.0), (np.nan, 5.0), (104.0, 69.5), (5.0, 5.0)])
    assert cs == [0, 1, 1, 1, 1, 1, 2] and ck == [6, 5]
    # no keypoint at all; one keypoint
    assert _table([]) == ([0] * 7, [])
    assert _table([(50.0, 50.0)]) == ([0, 0, 0, 0, 0, 1, 1], [0])


def test_cell_table_feeds_the_flat_prior_form_like_an_insertion_ordered_one():
    """with one 3-D neighbour per cell block the order inside a cell cannot matter: flat_stereo on the slot-order table equals
    flat_stereo on a table whose cells hold the same keypoints in reverse"""
    S = R.scenario("unrect-radtan")
    from oracle import oracle as O
    it = S["items"][0]
    f = it["frame"]
    keep = np.zeros(f["n"], bool)
    keep[np.nonzero(f["is3d"])[0][:1]] = True                           # a single 3-D keypoint: sums of one term
    state = (keep & (f["is3d"] != 0)).astype(np.uint8)
    unpx, bv = O.compute_keypoints(O.CAM_PINHOLE, S["K"], S["cfg"]["D"], S["iK"], f["px"])
    cs, ck = R.cell_tables(f["px"], S["cfg"]["w"], S["cfg"]["h"], R.CELL)
    rev = np.concatenate([ck[cs[c]:cs[c + 1]][::-1] for c in range(len(cs) - 1)]).astype(np.int32)
    item = dict(Tcw=R.T._inv7(it["Twc"]), px=f["px"], unpx=unpx, bv=bv, wpt=f["wpt"], state=state, cell_start=cs)
    a, b = PR.flat_stereo(S["priors"], dict(item, cell_kp=ck)), PR.flat_stereo(S["priors"], dict(item, cell_kp=rev))
    assert (a["has_prior"] == 2).sum() >= 1 and all(a[k].tobytes() == b[k].tobytes() for k in a)


@pytest.mark.parametrize("name", sorted(R.CONFIGS))
def test_the_scenario_takes_every_branch(name):
    cond = R.conditions(name)
    cfg = R.CONFIGS[name]
    for d in cond:
        print(name, d)
    total = {k: sum(d[k] for d in cond) for k in cond[0]}
    assert len(cond) == cfg["batch"] and all(d["n"] == cfg["n_inner"] + cfg["n_edge"] for d in cond)
    assert total["prior1"] >= 10, "priors from the map point"
    if cfg["rect"]:
        assert total["prior2"] == 0 and total["sad_accepted"] >= 10 and total["sad_rejected"] >= 3, "line-search priors accepted and rejected"
    else:
        assert total["prior2"] >= 10 and total["sad_accepted"] == total["sad_rejected"] == 0, "priors from the 3-D neighbours"
    assert total["retried"] >= 3, "a prior track that fails the one-level pass"
    assert total["gate_rejected"] >= 3, "tracks the epipolar gate rejects (the rolled band)"
    assert total["stereo_ok"] >= 20 and total["tri_ok"] >= 5, "stereo keypoints, and new 3-D points"
    assert total["matched_3d"] >= 3, "3-D keypoints that match and are not triangulated"
    assert total["reprojection"] >= 3, "the reprojection gate"
    if cfg["rect"]:
        # the reversed pair of item 1: matches right of the keypoint
        assert cond[1]["negative_disparity"] >= 3 and total["depth"] == 0
    else:
        # the same pair without rectification: the midpoint lies behind the cameras.  disp < 0 is a test of the rectified branch alone
        assert cond[1]["depth"] >= 3 and total["negative_disparity"] == 0
    if cfg["batch"] > 2:
        assert cond[2]["prior1"] == cond[2]["prior2"] == cond[2]["matched_3d"] == 0, "item 2 has no 3-D slot"


def test_the_route_fills_the_record_of_the_call():
    """the route's records carry the fields of ov2_stereo_keyframe_result, in its order, and its three actions"""
    assert R.REC_KEYS == ("action", "n", "n_prior3d", "n_prior_nb", "n_stereo_kps", "n_stereo", "n_stereo_good", "nb3dkps")
    assert (R.NOT_REQUESTED, R.NOT_KEYFRAME, R.DONE) == (0, 1, 2)
    recs, out = R.route(None, None, None, 2, [R.NOT_REQUESTED, R.NOT_KEYFRAME], R.scenario("rect"), None, R.empty_out(2, 4, 0x5A))
    assert recs == [dict(dict.fromkeys(R.REC_KEYS, 0), action=a) for a in (0, 1)]
    assert all((a.view(np.uint8) == 0x5A).all() for a in out.values())          # nobody asked, or nobody's keyframe: nothing is written


def test_rectified_depth_gate_is_out_of_reach():
    """the one branch no test reaches: with rectification z = fx |t| / |disp| and right.z = left.z (Trl is a pure
    x-translation), so left.z < 0.1 needs disp > fx |t| / 0.1: more than 0.6 of the image width"""
    cfg = R.CONFIGS["rect"]
    K, _ = R.camera(cfg)
    assert K[0] * R.BASELINE / 0.1 > 0.6 * cfg["w"] and all(d["depth"] == 0 for d in R.conditions("rect"))
