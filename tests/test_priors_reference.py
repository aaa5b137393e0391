"""tests/priors_ref.py against itself: the literal replay of the reference's loops (VisualFrontEnd::kltTracking :156-184,
MapManager::stereoMatching :396-489) and the flat per-keypoint form that csrc/priors.hip implements give the same bits on every
generated scene and every crafted case, and the generated scenes exercise every outcome."""
import numpy as np
import pytest

from tests import priors_ref as R

_CACHE = {}


def _scenes(form):
    """[(name, P, frame, mps, item, replay arrays, flat arrays, ev)], computed once"""
    if form not in _CACHE:
        out = []
        for name, P, frame, mps in R.scene_list(form):
            item = R.flatten(P, frame, mps)
            ev = {}
            if form == "klt":
                a, b = R.klt_arrays(frame, R.replay_klt(P, frame, mps)), R.flat_klt(P, item, ev)
            else:
                a, b = R.stereo_arrays(frame, R.replay_stereo(P, frame, mps)), R.flat_stereo(P, item, ev)
            out.append((name, P, frame, mps, item, a, b, ev))
        _CACHE[form] = out
    return _CACHE[form]


@pytest.mark.parametrize("form", ["klt", "stereo"])
def test_replay_equals_flat_bit_for_bit(form):
    scenes = _scenes(form)
    assert len(scenes) >= 24
    assert {len(s[6]["has_prior"]) for s in scenes} == set(R.SCENE_NS)
    assert {(s[1]["model"], 0 if s[1]["D"] is None else len(s[1]["D"])) for s in scenes} == {("pinhole", 0), ("pinhole", 4), ("pinhole", 8),
                                                                                           ("fisheye", 4)}
    assert {s[1]["rect"] for s in scenes} == {False, True} and {s[1]["klt_use_prior"] for s in scenes} == {False, True}
    for name, P, frame, mps, item, a, b, ev in scenes:
        ok, field = R.same(a, b)
        assert ok, (name, field)
        no = b["has_prior"] == 0
        assert np.array_equal(b["prior"][no].view(np.uint32), item["px"][no].view(np.uint32)), name     # px where there is no prior


def test_every_outcome_occurs_in_five_percent_of_the_keypoints():
    """a condition on the generators, met by the reference alone"""
    klt = np.concatenate([s[6]["has_prior"] for s in _scenes("klt")])
    share = {v: float((klt == v).mean()) for v in (0, 1)}
    print("frame form", len(klt), share)
    assert min(share.values()) >= 0.05, share
    st = _scenes("stereo")
    hp, sk = np.concatenate([s[6]["has_prior"] for s in st]), np.concatenate([s[6]["skip"] for s in st])
    share = {v: float((hp == v).mean()) for v in (0, 1, 2)}
    share["skip"] = float((sk != 0).mean())
    print("stereo form", len(hp), share)
    assert min(share.values()) >= 0.05, share
    # a 3-D keypoint whose right projection leaves the image and which then takes the neighbours' depth occurs in the scenes too
    assert sum(int(((s[6]["has_prior"] == 2) & (s[4]["state"] == 1)).sum()) for s in st) > 0
    # and the cell lists are not in keypoint order (the order of the sums is the cells')
    assert any(np.any(np.diff(s[4]["cell_kp"][s[4]["cell_start"][c]:s[4]["cell_start"][c + 1]]) < 0)
               for s in st for c in range(len(s[4]["cell_start"]) - 1))


def test_fisheye_scenes_keep_their_projections_away_from_the_image_edges():
    """what tests/test_gpu_priors.py relies on for the flags of the fisheye scenes (atan: one float ulp on the projection)"""
    n = 0
    for form in ("klt", "stereo"):
        for name, P, frame, mps, item, a, b, ev in _scenes(form):
            if P["model"] == "fisheye":
                assert ev.get("margin", np.inf) >= 1e-3, (name, ev)
                n += 1
    assert n >= 8


def _run_klt(case):
    name, P, frame, mps, exp = case
    item = R.flatten(P, frame, mps)
    a, b = R.klt_arrays(frame, R.replay_klt(P, frame, mps)), R.flat_klt(P, item)
    ok, field = R.same(a, b)
    assert ok, (name, field)
    assert b["has_prior"].tolist() == exp, (name, b["has_prior"])
    return item, b


def _run_stereo(case):
    name, P, frame, mps, exp, skip = case
    item = R.flatten(P, frame, mps)
    ev = {}
    a, b = R.stereo_arrays(frame, R.replay_stereo(P, frame, mps)), R.flat_stereo(P, item, ev)
    ok, field = R.same(a, b)
    assert ok, (name, field)
    assert b["has_prior"].tolist() == exp and b["skip"].tolist() == skip, (name, b["has_prior"], b["skip"])
    return item, b, ev


def test_crafted_frame_cases_show_what_they_were_crafted_for():
    cases = {c[0]: c for c in R.crafted_klt()}
    item, b = _run_klt(cases["behind_camera_projects_inside"])
    assert item["wpt"][0][2] < 0 and b["has_prior"][0] == 1                 # no depth gate: behind the camera, inside the image
    assert 0 <= b["prior"][0][0] < 768 and 0 <= b["prior"][0][1] < 512 and not np.array_equal(b["prior"][0], item["px"][0])
    item, b = _run_klt(cases["z_zero"])
    assert (item["wpt"][:, 2] == 0).all() and np.array_equal(b["prior"], item["px"])
    P = cases["z_zero"][1]
    with np.errstate(all="ignore"):
        p0, p1 = R.project_dist(P, (0.0, 0.0, 0.0)), R.project_dist(P, (1.0, 1.0, 0.0))
    assert np.isnan(p0[0]) and np.isinf(p1[0]) and not R.in_image(P, p0) and not R.in_image(P, p1)
    item, b = _run_klt(cases["exactly_on_img_w_and_on_0"])
    proj = [R.project_dist(P, tuple(w)) for w in item["wpt"]]
    assert proj[0][0] == 768 and proj[1][0] == 0 and proj[2][1] == 512 and proj[3][1] == 0      # exactly on the edges
    assert b["prior"][1][0] == 0 and b["prior"][3][1] == 0
    item, b = _run_klt(cases["klt_use_prior_off"])
    assert np.array_equal(b["prior"], item["px"])
    assert len(cases) == 4


def test_crafted_stereo_cases_show_what_they_were_crafted_for():
    cases = {c[0]: c for c in R.crafted_stereo()}
    item, b, ev = _run_stereo(cases["right_projection_leaves_then_neighbours"])
    P = cases["right_projection_leaves_then_neighbours"][1]
    own = R.project_dist(P, R.se3_act(R.pose(P["Tcic0"]), tuple(np.float64(v) for v in item["wpt"][0])))
    assert item["state"][0] == 1 and not R.in_image(P, own) and b["has_prior"][0] == 2
    item, b, ev = _run_stereo(cases["cell_row0_col0"])
    assert item["px"][0][0] < 32 and item["px"][0][1] < 32 and b["has_prior"][0] == 2
    item, b, ev = _run_stereo(cases["column_minus_one_not_wrapped"])
    nbw = R.grid_width(P)[0]
    assert item["cell_start"][nbw] - item["cell_start"][nbw - 1] == 1      # the last cell of row 0 holds the 3-D keypoint
    assert ev.get("alone") == 1 and b["has_prior"][0] == 0
    item, b, ev = _run_stereo(cases["alone_in_block"])
    assert ev.get("alone") == 1
    item, b, ev = _run_stereo(cases["coincident_unpx_nan"])
    assert np.array_equal(item["unpx"][0], item["unpx"][1]) and ev.get("nan_mean") == 1 and b["has_prior"][0] == 0
    item, b, ev = _run_stereo(cases["without_the_coincidence"])
    assert "nan_mean" not in ev and b["has_prior"][0] == 2
    item, b, ev = _run_stereo(cases["state2_and_as_neighbour"])
    assert item["state"][1] == 2 and b["skip"][1] == 1 and b["has_prior"][1] == 0 and ev.get("alone") == 1
    item, b, ev = _run_stereo(cases["state1_as_neighbour"])
    assert b["has_prior"][0] == 2 and "alone" not in ev
    item, b, ev = _run_stereo(cases["exactly_on_0_and_on_img_w"])
    proj = [R.project_dist(P, R.se3_act(R.pose(P["Tcic0"]), tuple(np.float64(v) for v in w))) for w in item["wpt"]]
    assert proj[0][0] == 0 and proj[1][0] == 768 and b["prior"][0][0] == 0 and np.array_equal(b["prior"][1], item["px"][1])
    item, b, ev = _run_stereo(cases["rect_stops_before_the_neighbours"])
    assert cases["rect_stops_before_the_neighbours"][1]["rect"] and b["has_prior"][0] == 0
    assert len(cases) == 10


def test_replay_klt_needs_the_map_point_of_every_3d_keypoint():
    """map_plms_.at(): the reference throws, the replay raises"""
    P = R.make_params(cam=R.CRAFT_CAM)
    frame, mps = R.toy(P, [(1, (300, 200), 2, None)])
    with pytest.raises(KeyError):
        R.replay_klt(P, frame, mps)
