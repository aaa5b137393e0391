"""The scenes of tests/kltfromkf_cases.py on the CPU oracle alone (tests/kltfromkf_ref.py): every branch of kltTrackingFromKF that
tests/test_gpu_kltfromkf.py means to compare is populated.  These are conditions on the cases, not measurements of the code: a
generator that misses one is changed, never the condition."""
import numpy as np
import pytest

from tests import kltfromkf_cases as KC
from tests import kltfromkf_ref as R


@pytest.fixture(scope="module")
def runs(oracle):
    """{(case, item index): (item, px, status, p3p)} -- computed once, changed by nobody"""
    out = {}
    for name in KC.NAMES:
        c = KC.case(name)
        for k, it in enumerate(c["items"]):
            out[(name, k)] = (it,) + KC.reference(oracle, it, c["use_prior"])
    return out


def test_the_generator_is_deterministic_and_in_range():
    for name in KC.NAMES:
        c = KC.case(name)
        assert len(c["items"]) == KC.N_ACTIVE < KC.BATCH
        for it in c["items"]:
            assert it["n"] <= KC.N_MAX and len(it["tab_lmid"]) <= KC.N_MAX
            assert np.all(np.diff(it["tab_lmid"]) > 0) and len(set(it["lmid"].tolist())) == it["n"]
            assert it["px"].dtype == np.float32 and np.isfinite(it["px"]).all() and np.isfinite(it["wpt"]).all()
    assert KC.item("mixed", 500)["px"].tobytes() == KC.item.__wrapped__("mixed", 500)["px"].tobytes()


def test_the_cases_populate_every_branch(oracle, runs, capsys):
    outside = {k: int((st & R.ST_NOT_IN_KF).astype(bool).sum()) for k, (it, px, st, p3p) in runs.items()}
    size = {k: it["n"] for k, (it, px, st, p3p) in runs.items()}
    with capsys.disabled():
        for k, (it, px, st, p3p) in runs.items():
            print("\n  %s[%d] %-8s n %3d, not in keyframe %3d, prior pass %3d, retried %3d (recovered %3d), tracked %3d, rule %d"
                  % (k[0], k[1], it["kind"], it["n"], outside[k], int((((st & 4) == 0) & (it["has_prior"] != 0) & KC.SPECS[k[0]]["use_prior"]).sum()),
                     int((st & 2).astype(bool).sum()), int(((st & 3) == 3).sum()), int((st & 1).sum()), p3p), end="")
        print()
    # membership: an item with some slots outside the keyframe, one with none, one with all
    assert any(0 < outside[k] < size[k] for k in runs) and any(outside[k] == 0 and size[k] > 0 for k in runs)
    assert any(outside[k] == size[k] and size[k] > 0 for k in runs)
    main = {k: v for k, v in runs.items() if k[0] != "noprior"}
    # a prior-pass failure that the retry recovers, and one that stays lost
    assert any(((st & 3) == 3).any() for (it, px, st, p3p) in main.values())
    assert any(((st & 3) == 2).any() for (it, px, st, p3p) in main.values())
    # the 33 % rule fires on an item and does not on another
    assert any(p3p for (it, px, st, p3p) in main.values()) and any(not p3p and (st & 2).any() for (it, px, st, p3p) in main.values())
    # sizes: an empty item and a full one
    assert any(n == 0 for n in size.values()) and any(n == KC.N_MAX for n in size.values())
    # klt_use_prior = 0: nothing enters the prior pass, nothing is retried, the rule cannot fire
    for k, (it, px, st, p3p) in runs.items():
        if k[0] == "noprior":
            assert not p3p and not (st & 2).any()
    assert any(k[0] == "noprior" and (st & 1).any() for k, (it, px, st, p3p) in runs.items())
    # a slot outside the keyframe keeps its px and is never tracked
    for it, px, st, p3p in runs.values():
        out = (st & 4) != 0
        assert np.array_equal(st[out], np.full(out.sum(), 4, np.uint8)) and px[out].tobytes() == it["px"][out].tobytes()


def test_the_cases_tell_the_two_retry_rules_and_the_two_starts_apart(oracle, runs):
    """kltTracking retries a lost prior track from the first pass's forward result and starts a slot without a prior from its source
    point; kltTrackingFromKF uses the frame's own px for both.  A kernel that took the other rule would pass unnoticed unless a slot's
    result bits differ between the two: at least one does, for each."""
    retry = nopri = 0
    for (name, k), (it, px, st, p3p) in runs.items():
        if p3p or not it["n"]:
            continue                                  # (where the rule fired every second-call prior was reset: the starts do not show)
        use = KC.SPECS[name]["use_prior"]
        px_f, st_f, _ = KC.reference(oracle, it, use, retry_from="forward")
        sel = (st & 2) != 0
        retry += int((px_f[sel].view(np.uint32) != px[sel].view(np.uint32)).any(axis=1).sum())
        px_k, st_k, _ = KC.reference(oracle, it, use, noprior_from="kf")
        sel = (st & 6) == 0
        sel &= ~((it["has_prior"] != 0) & use)
        nopri += int((px_k[sel].view(np.uint32) != px[sel].view(np.uint32)).any(axis=1).sum())
    assert retry >= 1 and nopri >= 1, (retry, nopri)
