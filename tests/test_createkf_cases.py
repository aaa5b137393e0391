"""The rounds of tests/createkf_cases.py do what they are named for, asserted on the CPU oracle, tests/kfreq_ref.py and
tests/brief_ref.py alone (no GPU, no library call): every item has the noccupcells, the sign of nb2detect and the oracle's n_new its
case needs; the frames claimed to carry invalid descriptors do; the crowded item overflows the 160 slots and no other item does.  The
adaptive state is carried from round to round by the oracle's own rule, as the GPU test carries it."""
import numpy as np
import pytest

from tests import brief_ref
from tests import createkf_cases as CC
from tests import createkf_ref as CR

_REPLAY = {}


def _replay(O, detector):
    """-> per round, per active item: dict(n_prev, noccupcells, nb2detect, n_new, invalid, dup, flag)"""
    if detector in _REPLAY:
        return _REPLAY[detector]
    state = [CC.FAST_TH0 if detector == "gridfast" else CC.QUALITY0] * CC.BATCH
    rounds = []
    for ri, r in enumerate(CC.ROUNDS):
        p, x = CC.round_params(r, detector), CC.round_inputs(ri)
        items = []
        for b in range(r["n_active"]):
            m = int(x["n"][b])
            px = x["px"][b, :m]
            nocc, nb3d = CR.counts(p, px, x["is3d"][b, :m])
            d = dict(n_prev=m, noccupcells=nocc, nb3dkps=nb3d, nb2detect=p["nbmaxkps"] - nocc, n_new=0, flag=int(x["make_kf"][b]),
                     invalid=int((~brief_ref.border_valid(px, CC.W, CC.H)).sum()), dup=len(set(x["lmid"][b, :m].tolist())) < m)
            if d["flag"] and d["nb2detect"] > 0:
                img = CC.frames()[b][0][r["frame"]]
                if detector == "gridfast":
                    with O.fast_tie_mode(O.FAST_TIE_LIBSTDCXX):
                        pts, state[b] = O.detect_grid_fast(img, p["det_cell"], px, state[b], p["mask_mode"], p["do_subpix"])
                else:
                    pts, state[b] = O.detect_singlescale(img, p["det_cell"], px, p["roi"], state[b], p["do_subpix"])
                d["n_new"] = len(pts)
            items.append(d)
        rounds.append(items)
    _REPLAY[detector] = rounds
    return rounds


def _round(rounds, name):
    return rounds[[r["name"] for r in CC.ROUNDS].index(name)]


@pytest.mark.parametrize("detector", ["singlescale", "gridfast"])
def test_rounds_reach_what_they_are_named_for(oracle, detector):
    rounds = _replay(oracle, detector)
    for r, items in zip(CC.ROUNDS, rounds):
        print(detector, r["name"], [(d["n_prev"], d["noccupcells"], d["nb2detect"], d["n_new"], d["invalid"]) for d in items])
    cap = (2 if detector == "singlescale" else 1) * (CC.W // CC.CELL) * (CC.H // CC.CELL)
    assert cap == (120 if detector == "singlescale" else 60)
    # the first frame: nothing tracked, every cell free, the detector fills the frame
    for d in _round(rounds, "first"):
        assert (d["n_prev"], d["noccupcells"], d["nb2detect"]) == (0, 0, 60) and 20 <= d["n_new"] <= min(cap, CC.N_MAX)
    # few cells occupied: the detector tops up; every cell occupied: nothing to detect; unflagged between two flagged; the crowd overflows
    few, full, idle, crowd = _round(rounds, "mixed")
    assert 0 < few["noccupcells"] <= 12 and few["nb2detect"] >= 48 and few["n_new"] >= 10 and few["n_prev"] + few["n_new"] <= CC.N_MAX
    assert few["invalid"] >= 3 and few["invalid"] < few["n_prev"]                 # descriptors of both kinds in one frame
    assert full["noccupcells"] == 77 and full["nb2detect"] <= 0 and full["n_new"] == 0 and full["flag"] == 1
    assert idle["flag"] == 0 and idle["n_prev"] > 0
    assert crowd["n_prev"] == 150 and crowd["nb2detect"] > 0 and crowd["n_prev"] + crowd["n_new"] > CC.N_MAX
    # n_active < batch, a repeated id on a frame that detects, an unflagged item in the middle
    dup, idle2, asc = _round(rounds, "short")
    assert len(_round(rounds, "short")) == 3 < CC.BATCH and dup["dup"] and dup["n_new"] > 0 and idle2["flag"] == 0 and not asc["dup"] and asc["n_new"] > 0
    # the keyframe sizes around the sort's padding: nothing is detected in these rounds
    assert [d["n_prev"] for d in _round(rounds, "sizes")] == [1, 2, 64, 65] and [d["n_prev"] for d in _round(rounds, "full")] == [160, 128, 129, 0]
    assert all(d["nb2detect"] <= 0 and d["n_new"] == 0 for name in ("sizes", "full") for d in _round(rounds, name))
    assert CC.N_MAX == 160 and _round(rounds, "full")[0]["n_prev"] == CC.N_MAX
    # the overflow is the crowd's alone, the repeated id the one item's
    for r, items in zip(CC.ROUNDS, rounds):
        for b, d in enumerate(items):
            assert (d["n_prev"] + d["n_new"] > CC.N_MAX) == (r["name"] == "mixed" and b == 3), (r["name"], b)
            assert d["dup"] == (r["name"] == "short" and b == 0), (r["name"], b)
    # the keyframes the last round installs have points to track: every item detects or carries a full grid
    assert all(d["n_prev"] + d["n_new"] >= 40 for d in _round(rounds, "last"))


def test_slot_orders_and_shapes():
    orders = {it.get("order") for r in CC.ROUNDS for it in r["items"] if it["kind"] != "empty"}
    assert orders == {"desc", "random", "asc"}
    for ri, r in enumerate(CC.ROUNDS):
        x = CC.round_inputs(ri)
        for b, it in enumerate(r["items"]):
            m = int(x["n"][b])
            ids = x["lmid"][b, :m]
            assert (ids >= 0).all() and (ids < x["nlmid"][b]).all()
            if m > 2 and not it.get("dup"):
                d = np.diff(ids)
                assert {"desc": (d < 0).all(), "asc": (d > 0).all(), "random": (d < 0).any() and (d > 0).any()}[it["order"]], (r["name"], b)
    assert (CC.W, CC.H, CC.BATCH, CC.N_MAX, CC.CELL) == (376, 240, 4, 160, 35)
    assert {r["twc"] for r in CC.ROUNDS} == {"given", "resident"} and any(not CC.round_params(r, "singlescale")["use_brief"] for r in CC.ROUNDS)
