"""CPU test: the NumPy restatement of Tracking::UpdateLocalMap (tests/local_map_host.py) against tests/golden/local_map_ref.npz, which tools/gen_golden_local_map.py
wrote from the REAL reference lines.  Every list must be identical, and each case must hold what its name promises."""
import numpy as np
import pytest

import local_map_cases as LC
import local_map_host as LH


@pytest.fixture(scope="module")
def gold():
    return LH.golden()


@pytest.mark.parametrize("name", LC.NAMES)
def test_restatement_equals_the_reference(gold, name):
    case = LC.make(name)
    for f in range(len(case["frames"])):
        want, got = LH.golden_frame(gold, name, f), LH.host_frame(case, f)
        for k in LH.KEYS:
            assert np.array_equal(got[k], want[k]), (name, f, k)


def frames(gold, name):
    case = LC.make(name)
    return case, [LH.golden_frame(gold, name, f) for f in range(len(case["frames"]))]


def test_cases_hold_what_their_names_promise(gold):
    case, (r,) = frames(gold, "ties_and_bad_max")
    M = case["maps"][0]
    votes = {}
    for p in r["match"][r["match"] >= 0]:
        for k in M["obs"][p]:
            votes[k] = votes.get(k, 0) + 1
    top = max(votes, key=votes.get)
    assert M["kf_bad"][top] and top not in r["local_kf"]
    tied = [k for k in votes if votes[k] == votes[r["ref_kf"]] and not M["kf_bad"][k]]
    assert len(tied) == 2 and r["ref_kf"] == min(tied, key=lambda k: M["kf_rank"][k])

    case, rs = frames(gold, "empty_vote_keeps_previous")
    for F, r in zip(case["frames"], rs):
        assert r["ref_kf"] == -1 and r["local_kf"].tolist() == F["local_in"] and len(r["lp"]) > 0 and (r["match"] == -1).all()
    assert (case["frames"][1]["match"] >= 0).all()

    case, (r,) = frames(gold, "parent_ends_the_loop")
    M = case["maps"][0]
    voted = [k for k in r["local_kf"][:4]]
    assert r["local_kf"].tolist() == voted + [int(M["covis"][voted[0], 0]), int(M["parent"][voted[1]])]

    case, (r,) = frames(gold, "neighbour_child_choice")
    M = case["maps"][0]
    assert len(r["local_kf"]) == 3 + 5 and M["kf_bad"][r["local_kf"][-1]] and r["local_kf"][-1] == M["parent"][r["local_kf"][2]]

    case, rs = frames(gold, "cap_80")
    assert [len(r["local_kf"]) for r in rs] == [81, 90]

    case, (r,) = frames(gold, "dedupe_across_chunks")
    M = case["maps"][0]
    walk = np.concatenate([M["pts"][k] for k in r["local_kf"]])
    assert len(r["local_kf"]) == 3 and len(walk) == 4500
    pos = {int(p): i for i, p in reversed(list(enumerate(walk)))}
    late = [i for i, p in enumerate(walk) if p >= 0 and not M["pt_bad"][p] and pos[int(p)] < i]
    # duplicates whose first occurrence lies in an earlier chunk, for every chunk size up to 4096
    for chunk in (64, 256, 1024, 1500, 2048, 4096):
        assert any(pos[int(walk[i])] // chunk < i // chunk for i in late), chunk
    assert (walk == -1).any() and M["pt_bad"][walk[walk >= 0]].any() and len(set(r["lp"].tolist())) == len(r["lp"])

    case, rs = frames(gold, "shared_map_batch")
    assert len(rs) == 5 and len({F["map"] for F in case["frames"]}) == 2 and len({tuple(r["local_kf"]) for r in rs}) > 2

    case, (r,) = frames(gold, "lines")
    M = case["maps"][0]
    walk = np.concatenate([M["lines"][k] for k in r["local_kf"]])
    assert len(r["ll"]) < len(walk[walk >= 0]) and r["ll_seen"].any() and not r["ll_seen"].all()
    assert M["ml_bad"][walk[walk >= 0]].any() and (r["line_match"] != case["frames"][0]["line_match"]).any()

    case, (r,) = frames(gold, "wide_lists")
    M = case["maps"][0]
    assert case["expect_listed"][0] in r["local_kf"] and M["nk"] > 256 and len(case["frames"][0]["match"]) > 256
    hub = [k for k in range(M["nk"]) if len(M["children"][k]) > 64]
    assert hub and hub[0] in r["local_kf"]
