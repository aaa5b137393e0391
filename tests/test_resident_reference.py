"""tests/resident_ref.py: apply_ops, the numpy specification of ov2_btracker_update_frame, on hand-written frames (no GPU)."""
import numpy as np
import pytest

from ov2slam_amd import _lib as L
from tests import resident_ref as RR

SET, UNSET, REMOVE = L.OV2_RES_SET_POINT, L.OV2_RES_UNSET_POINT, L.OV2_RES_REMOVE


def _frame(n, first_id=100):
    """slot i: px (i, 2 i), distinct unsorted lmids from first_id on, every third slot 3-D with wpt (i, -i, 1)"""
    i = np.arange(n)
    lmid = first_id + np.random.default_rng(n).permutation(5 * n)[:n]
    return RR.make_frame(np.stack([i, 2 * i], 1), lmid, i % 3 == 0, np.stack([i, -i, np.ones(n)], 1))


def test_set_unset_and_remove_on_a_small_frame():
    f = _frame(6)
    f["lmid"][:] = [100, 107, 114, 121, 128, 105]
    assert f["lmid"].tolist() == [100, 107, 114, 121, 128, 105] and f["is3d"].tolist() == [1, 0, 0, 1, 0, 0]
    g, r = RR.apply_ops(f, [(114, SET, (1.5, 2.5, 3.5)), (121, UNSET, None), (107, REMOVE, None), (128, REMOVE, None), (100, SET, (9., 8., 7.))])
    assert r == dict(n_before=6, n_after=4, n_set=2, n_unset=1, n_removed=2, n_missing=0)
    # the remaining slots close up IN SLOT ORDER and keep their px
    assert g["n"] == 4 and g["lmid"].tolist() == [100, 114, 121, 105] and g["px"].tolist() == [[0, 0], [2, 4], [3, 6], [5, 10]]
    assert g["is3d"].tolist() == [1, 1, 0, 0]
    assert g["wpt"][0].tolist() == [9., 8., 7.] and g["wpt"][1].tolist() == [1.5, 2.5, 3.5]
    assert g["wpt"][2].tolist() == [3., -3., 1.]                         # UNSET keeps the point in the slot
    # the input is not modified
    assert f["n"] == 6 and f["is3d"].tolist() == [1, 0, 0, 1, 0, 0] and f["wpt"][0].tolist() == [0., 0., 1.]


def test_an_id_the_frame_does_not_hold_is_counted_and_changes_nothing():
    f = _frame(5)
    g, r = RR.apply_ops(f, [(999, SET, (1., 2., 3.)), (998, REMOVE, None), (997, UNSET, None)])
    assert r == dict(n_before=5, n_after=5, n_set=0, n_unset=0, n_removed=0, n_missing=3)
    assert RR.frame_bytes(g) == RR.frame_bytes(f) and g["wpt"].tobytes() == f["wpt"].tobytes()


def test_an_empty_op_list_and_an_empty_frame():
    f = _frame(7)
    g, r = RR.apply_ops(f, [])
    assert r == dict(n_before=7, n_after=7, n_set=0, n_unset=0, n_removed=0, n_missing=0) and RR.frame_bytes(g) == RR.frame_bytes(f)
    e, r = RR.apply_ops(RR.empty_frame(), [(1, SET, (0., 0., 1.)), (2, REMOVE, None)])
    assert e["n"] == 0 and r == dict(n_before=0, n_after=0, n_set=0, n_unset=0, n_removed=0, n_missing=2)
    e, r = RR.apply_ops(RR.empty_frame(), [])
    assert e["n"] == 0 and r["n_after"] == 0


@pytest.mark.parametrize("n", [160, 2048])
def test_a_full_frame(n):
    f = _frame(n)
    rng = np.random.default_rng(n)
    gone = rng.permutation(n)[:n // 3]
    moved = [i for i in rng.permutation(n)[:n // 2] if i not in set(gone.tolist())]
    ops = [(int(f["lmid"][i]), REMOVE, None) for i in gone] + [(int(f["lmid"][i]), SET, (float(i), 0.5, 2.)) for i in moved]
    ops = [ops[k] for k in rng.permutation(len(ops))]
    g, r = RR.apply_ops(f, ops)
    keep = np.ones(n, bool); keep[gone] = False
    assert r == dict(n_before=n, n_after=n - len(gone), n_set=len(moved), n_unset=0, n_removed=len(gone), n_missing=0)
    assert g["lmid"].tolist() == f["lmid"][keep].tolist() and g["px"].tobytes() == f["px"][keep].tobytes()
    want3d = f["is3d"].copy(); want3d[moved] = 1
    assert g["is3d"].tolist() == want3d[keep].tolist()
    # a REMOVE list that holds every id empties the frame
    e, r = RR.apply_ops(f, [(int(v), REMOVE, None) for v in f["lmid"]])
    assert e["n"] == 0 and r["n_removed"] == n and len(e["px"]) == len(e["lmid"]) == len(e["is3d"]) == len(e["wpt"]) == 0


def test_a_repeated_id_in_one_list_and_an_unknown_op_are_errors():
    f = _frame(4)
    with pytest.raises(AssertionError):
        RR.apply_ops(f, [(100, SET, (1., 1., 1.)), (100, REMOVE, None)])
    with pytest.raises(ValueError):
        RR.apply_ops(f, [(100, 7, None)])
