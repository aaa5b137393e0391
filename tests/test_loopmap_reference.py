"""The specification of the loop closer's local-map tracking (tests/loopmap_ref.py) against itself and against its neighbours, on
the CPU: the literal replay of LoopCloser::trackLoopLocalMap / matchToMap equals the flat per-point form on the flattened arrays,
bit for bit, over a campaign that reaches every status, every candidate gate, both tie sites and both effects of the matched flag;
the set-building walk; the known answers of the multiplied viewing cone; and the flat form against the mapper's
(tests/match_ref.py) where the two functions coincide."""
import numpy as np
import pytest

from tests import loopmap_ref as R
from tests import match_ref as MR

CALIBS = {"nodist": dict(D=None), "radtan4": dict(D=R.RADTAN4), "radtan5": dict(D=R.RADTAN5),
          "fisheye": dict(D=R.FISHEYE4, model="fisheye")}
SEEDS = range(6)                                                        # 4 calibrations x 6 seeds = 24 scenes


@pytest.fixture(scope="module")
def campaign():
    """every scene once: (P, M, item, meta, flat result, flat events, replay result, replay's vkplmids, replay events)"""
    runs = []
    for c, (name, kw) in enumerate(CALIBS.items()):
        P = R.make_params(**kw)
        for seed in SEEDS:
            M = R.make_scene(P, np.random.default_rng(100 * c + seed))
            item, meta = R.flatten(M)
            ev_f, ev_r = {}, {}
            f = R.flat(P, item, ev_f)
            ra, vk = R.replay_arrays(M, meta, ev_r)
            runs.append(dict(name="%s-%d" % (name, seed), P=P, M=M, item=item, meta=meta, flat=f, ev_f=ev_f, replay=ra, vk=vk, ev_r=ev_r))
    return runs


def test_replay_equals_flat_of_flatten_on_every_field(campaign):
    assert len(campaign) >= 24
    for run in campaign:
        ok, field = R.same(run["replay"], run["flat"])
        assert ok, (run["name"], field)
        assert run["vk"] == R.vkplmids_of(run["flat"], run["meta"]), run["name"]
        new = run["vk"][len(run["meta"]["walk_vkplmids"]):]
        assert [k for k, _ in new] == sorted(k for k, _ in new) and len(new) == run["flat"]["n_matches"], run["name"]


def test_campaign_reaches_every_status_gate_and_tie(campaign):
    seen = set()
    tot_f, tot_r = {}, {}
    for run in campaign:
        seen |= set(int(s) for s in run["flat"]["lm_status"])
        for tot, ev in ((tot_f, run["ev_f"]), (tot_r, run["ev_r"])):
            for k, v in ev.items():
                tot[k] = tot.get(k, 0) + v if k != "margin" else 0
    assert seen == {R.BEHIND, R.OUT_OF_FOV, R.OUT_OF_IMAGE, R.NO_CANDIDATE, R.RATIO_REJECTED, R.BEST}
    for gate in ("gate_matched", "gate_nomp", "gate_pxdist", "gate_shared", "tie_best", "tie_pick"):
        assert tot_f.get(gate, 0) > 0 and tot_r.get(gate, 0) > 0, gate
    for gate in ("gate_matched", "gate_shared", "tie_best", "tie_pick"):
        assert tot_f[gate] == tot_r[gate], gate                        # (the pixel gate sits before the map-point lookup in one form, behind it in the other)
    for step in ("walk_below", "walk_above", "walk_missing", "walk_erased"):
        assert tot_r.get(step, 0) > 0, step


def test_campaign_reaches_both_effects_of_the_matched_flag(campaign):
    take = unrej = 0
    for run in campaign:
        t, u = R.matched_flag_effects(run["P"], run["item"])
        take += len(t); unrej += len(u)
        assert run["item"]["kp_matched"].sum() > 0.2 * len(run["item"]["kp_matched"])
    assert take > 0, "no point whose best keypoint was excluded with the second taking over"
    assert unrej > 0, "no point that the exclusion turns from RATIO_REJECTED into BEST"


@pytest.mark.parametrize("case", R.crafted_cases(), ids=lambda c: c[0])
def test_crafted_cases_in_both_forms(case):
    name, M, status, lm_kp = case
    item, meta = R.flatten(M)
    f = R.flat(M["params"], item)
    assert [int(s) for s in f["lm_status"]] == status
    assert [int(k) for k in f["lm_kp"]] == lm_kp
    ra, vk = R.replay_arrays(M, meta)
    ok, field = R.same(ra, f)
    assert ok, field
    assert vk == R.vkplmids_of(f, meta)


def test_matched_flag_effects_on_the_crafted_cases():
    cases = {c[0]: c[1] for c in R.crafted_cases()}
    item, _ = R.flatten(cases["matched_best_excluded_second_takes_over"])
    t, u = R.matched_flag_effects(cases["matched_best_excluded_second_takes_over"]["params"], item)
    assert list(t) == [0] and len(u) == 0
    item, _ = R.flatten(cases["matched_exclusion_unrejects"])
    t, u = R.matched_flag_effects(cases["matched_exclusion_unrejects"]["params"], item)
    assert len(t) == 0 and list(u) == [0]


# ---- the set-building walk ---------------------------------------------------------------------------------------------------------------
def _walk_map(cov, cokfs, observed=(), vkplmids=(), lc=100):
    mps = {i: dict(is3d_=True, wpt=np.array([0.0, 0.0, -1.0]), set_kfids_=[1], map_kf_desc_={1: np.zeros(32, np.uint8)})
           for ids in cokfs.values() for i in ids}
    nbw, nbh = R.grid_width(R.make_params())
    return dict(params=R.make_params(), newkf=dict(kfid_=500, mapkps_={i: (np.float32(10), np.float32(10)) for i in observed},
                                                   vgridkps_=[[] for _ in range(nbw * nbh)]),
                Tcw=np.array([0, 0, 0, 0, 0, 0, 1.0]), lckf=dict(kfid_=lc, cov=cov), cokfs=cokfs, mps=mps, vkplmids=list(vkplmids),
                local_order=None)


def test_walk_window_continue_below_break_above():
    cokfs = {84: [1], 85: [2], 100: [3], 115: [4], 116: [5], 130: [6]}
    M = _walk_map({k: 10 for k in cokfs}, cokfs)
    vk, info = R.replay(M)
    assert info["local"] == [2, 3, 4] and vk == []
    assert R.local_set(M) == ([], [2, 3, 4])


def test_walk_skips_a_missing_keyframe_and_always_takes_the_loop_keyframe():
    cokfs = {98: [1, 2], 100: [7, 8]}
    M = _walk_map({98: 10, 99: 30}, cokfs)                              # 99 is in the covisibility map, not in the map; 100 is not in its own map
    vk, info = R.replay(M)
    assert info["local"] == [1, 2, 7, 8]
    assert R.local_set(M)[1] == [1, 2, 7, 8]


def test_walk_pairs_observed_points_once_and_erases_paired_points():
    cokfs = {99: [1, 2, 3, 2], 100: [3, 4, 5, 1]}
    # the new keyframe observes 2 and 4; (4, 4) is already in vkplmids; keypoint 9 was paired with local point 5 by an earlier stage
    M = _walk_map({99: 10}, cokfs, observed=(2, 4, 9), vkplmids=[(4, 4), (9, 5)])
    vk, info = R.replay(M)
    assert info["walk_vkplmids"] == [(4, 4), (9, 5), (2, 2)]
    assert info["local"] == [1, 3]                                      # 5 erased, 2 and 4 never entered
    assert R.local_set(M) == ([(4, 4), (9, 5), (2, 2)], [1, 3])
    assert vk == info["walk_vkplmids"]                                  # every local point is behind the camera: nothing is appended
    item, meta = R.flatten(M)
    assert list(item["kp_matched"]) == [1, 1, 1] and meta["lm_lmid"] == [1, 3]


def test_walk_order_list_decides_the_iteration():
    cokfs = {100: [1, 2, 3, 4]}
    M = _walk_map({}, cokfs)
    M["local_order"] = [3, 1]
    assert R.replay(M)[1]["local"] == [3, 1, 2, 4]


# ---- known answers -----------------------------------------------------------------------------------------------------------------------
def test_euroc_view_threshold_known_answer():
    view_th, dmax, mindist = R.thresholds(R.make_params())
    assert view_th.dtype == np.float32 and view_th == np.float32(5.797544e-06)
    assert dmax == np.float32(10) and mindist == np.float32(np.float64(np.float32(32) * np.float32(np.float32(0.2 * 1.5))) * 8.0)
    # the same for a calibration whose vfov would be the larger one: atan(hfov) in both branches
    tall = R.make_params(cam=dict(R.EUROC, K=(100.0, 900.0, 367.215, 248.375)))
    assert R.thresholds(tall)[0] == np.float32(np.cos(np.float64(np.float32(np.arctan(np.float64(np.float32(0.5 * 752 * 100.0)))))))


def test_viewing_cone_known_points():
    case = {c[0]: c for c in R.crafted_cases()}["out_of_fov_and_out_of_image"]
    item, _ = R.flatten(case[1])
    f = R.flat(case[1]["params"], item)
    assert list(f["lm_status"]) == [R.OUT_OF_FOV, R.OUT_OF_IMAGE]
    assert tuple(f["lm_projpx"][0]) == (0.0, 0.0) and f["lm_projpx"][1][0] > 752


# ---- the two specifications side by side ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("calib", ["nodist", "radtan4"])
def test_flat_agrees_with_the_mappers_flat_where_the_functions_coincide(calib):
    """No matched flags, nb3dkps >= 30, equal fmaxprojerr / fdistratio, every observation stale (the Mapper's re-projection gate
    then passes by its NaN rule), and without the points the Mapper's narrower viewing cone removes: every field agrees."""
    P = MR.make_params(fmax_proj_pxdist=10.0, fmax_desc_dist=R.FDISTRATIO, **CALIBS[calib])
    M = MR.make_scene(P, np.random.default_rng(5), n_kp=120, n_lm=261, nb3dkps=100)
    kf, _ = MR.flatten(M)
    kf["obs_kf"] = np.full_like(kf["obs_kf"], -1)
    kf["obs_px"] = np.zeros_like(kf["obs_px"])
    keep = MR.flat(P, kf)["lm_status"] != MR.OUT_OF_FOV
    assert 0 < (~keep).sum() < len(keep)
    kf["lm_mp"], kf["lm_wpt"] = kf["lm_mp"][keep], kf["lm_wpt"][keep]
    want = MR.flat(P, kf)
    item = {k: kf[k] for k in ("Tcw", "kp_px", "kp_mp", "cell_start", "cell_kp", "obs_start", "obs_kfid", "desc_start", "desc", "lm_mp", "lm_wpt")}
    item["kp_matched"] = np.zeros(len(kf["kp_mp"]), np.uint8)
    got = R.flat(P, item)
    ok, field = R.same(got, want)
    assert ok, field
    assert want["n_matches"] > 5 and (want["lm_status"] == R.RATIO_REJECTED).any() and not (got["lm_status"] == R.OUT_OF_FOV).any()
