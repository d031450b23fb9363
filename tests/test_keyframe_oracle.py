"""CPU test: the NumPy restatement of the key-frame insertion calls (tests/keyframe_host.py, which walks serially as the reference does) against what the real
reference lines left in tests/golden/keyframe_ref.npz (tools/gen_golden_keyframe.py), every integer and every flag; the outcome each decision case is named for;
the closed form of CreateNewKeyFrame's walk against the serial walk; the capacity and twice-named rules on the restatement."""
import numpy as np
import pytest

import keyframe_cases as KC
import keyframe_check as CK
import keyframe_host as KH
from planarslam_amd import keyframe as KF


def test_the_fixture_holds_every_case_the_reference_can_run():
    with np.load(CK.GOLDEN) as z:
        assert set(z.files) == set(KC.REF_NAMES)


@pytest.mark.parametrize("name", KC.REF_NAMES)
def test_restatement_agrees_with_the_reference(name):
    case = KC.make(name)
    before = KC.pack(case)
    after, out = CK.run_host(case, before)
    CK.check_against_ref(case, before, after, out)


@pytest.mark.parametrize("name", [n for n in KC.NAMES if n.startswith("need_")])
def test_decision_cases_catch_what_they_are_named_for(name):
    case = KC.make(name)
    _, out = CK.run_host(case)
    for k, v in case["expect"].items():
        assert out[0, KF.OUT_FIELDS.index(k)] == v, (k, dict(zip(KF.OUT_FIELDS, out[0].tolist())))


@pytest.mark.parametrize("name", [n for n in KC.NAMES if KC.kind(n) == "create" and "short" not in n])
def test_closed_form_of_the_walk(name):
    """the serial walk with its break processes the first min(M, max(100, c) + 1) candidates in sorted order; the lines the first min(ML, 51)"""
    case = KC.make(name)
    for b, F in enumerate(case["frames"]):
        M, th = case["maps"][F["map"]], case["th_depth"][b]
        for z, match, nobs, points in ((F["depth"], F["match"], M["pt_nobs"], True), (F["depth_line"], F["lmatch"], M["ml_nobs"], False)):
            cand = sorted((float(z[i]), i) for i in range(len(z)) if z[i] > 0)
            c = sum(1 for zz, _ in cand if not np.float32(zz) > th)
            proc = min(len(cand), max(100, c) + 1) if points else min(len(cand), 51)
            want = [i for _, i in cand[:proc] if match[i] == -1 or nobs[match[i]] < 1]
            assert KH._walk(z, match, nobs, th, points) == want


def test_walk_boundaries_are_what_the_cases_say():
    n = lambda name: int(CK.run_host(KC.make(name))[1]["n_created_pt"][0])
    assert [n(f"walk_close_{m}") for m in (0, 1, 99, 100, 101, 102)] == [0, 1, 99, 100, 101, 102]
    assert [n(f"walk_far_{m}") for m in (0, 1, 99, 100, 101, 102)] == [0, 1, 99, 100, 101, 101]
    assert [n(f"walk_c_{c}") for c in (99, 100, 101, 150)] == [101, 101, 102, 151]
    assert n("walk_at_threshold") == 131 and n("walk_ties") == 101
    nl = lambda name: int(CK.run_host(KC.make(name))[1]["n_created_ml"][0])
    assert nl("lines_0") == 0 and nl("lines_50") <= 50 and nl("lines_52") <= 51


@pytest.mark.parametrize("name", [n for n in KC.NAMES if "_short_" in n or n.endswith("_twice")])
def test_capacity_and_twice_named_leave_everything_as_it_was(name):
    case = KC.make(name)
    before = KC.pack(case)
    after, out = CK.run_host(case, before)
    if "_short_" in name:
        assert out["status"].tolist() == [3]
        CK.check_same_state(before, after, name)
    else:
        assert sorted(out["status"].tolist()) == [0, 2, 2]
        g = 0                                                                # the map named twice
        for k, a in before["map"].items():
            CK.same(a[g], after["map"][k][g], k)
