"""CPU: the host restatement of the key-frame database queries (tests/host_shim/kfdb_host.cpp) equals, bit for bit, what the REAL reference gave on the same seeded
cases (tests/golden/kfdb_ref.npz, written by tools/gen_golden_kfdb.py from src/KeyFrameDatabase.cc and the vendored DBoW2), and the cases reach every exit and every
reference behaviour the device code has to keep."""
import numpy as np
import pytest

import kfdb_cases as KC
import kfdb_host as KH

MODE_EXITS = {0: ("not_sharing", "word_threshold", "not_retained", "duplicate", "candidate"),               # reloc: nothing is excluded, there is no minScore
              1: ("not_sharing", "excluded", "word_threshold", "below_min_score", "not_retained", "duplicate", "candidate")}


@pytest.fixture(scope="module")
def runs():
    L = KH.load_host()
    return {name: (KC.build(name),) + KH.host_case(L, KC.build(name)) for name in KC.CASES}


@pytest.mark.parametrize("name", list(KC.CASES))
def test_restatement_equals_the_real_reference(runs, name):
    G = KH.golden()
    case, db, res = runs[name]
    assert len(res) == len(G[name + "_n_cand"])
    for q, r in enumerate(res):
        # the state the scores carry from query to query, then the outputs
        assert r["score_in"].view(np.uint32).tolist() == G[name + "_score_in"][q].view(np.uint32).tolist(), q
        assert r["n_cand"] == G[name + "_n_cand"][q], q
        assert r["cand"][:r["n_cand"]].tolist() == G[name + "_cand"][q][:r["n_cand"]].tolist(), q
        assert r["common"].tolist() == G[name + "_common"][q].tolist(), q
        assert r["score"].view(np.uint32).tolist() == G[name + "_score"][q].view(np.uint32).tolist(), q
        assert r["n_scored"] == G[name + "_n_scored"][q], q


@pytest.mark.parametrize("name", list(KC.CASES))
def test_pair_scores_are_the_references_doubles(name):
    G = KH.golden()
    case = KC.build(name)
    pairs = KC.score_pairs(case)
    got, _ = KH.host_bow_score(KH.load_host(), [KC.bow_of(case, a) + KC.bow_of(case, b) for a, b in pairs])
    assert got.view(np.uint64).tolist() == G[name + "_pair_score"].view(np.uint64).tolist()
    assert abs(got[-1] - 1.0) < 1e-12 and (got[:-1] < 0.999).all() and (got > 0).any()      # the last pair is a vector against itself: the data is not degenerate


def test_every_exit_is_reached_in_both_modes(runs):
    seen = {0: set(), 1: set()}
    for case, db, res in runs.values():
        for q, r in zip(case["queries"], res):
            seen[q["mode"]] |= {KH.EXITS[e] for e in r["exits"][:case["n_kf"]]}
    for mode, want in MODE_EXITS.items():
        assert seen[mode] == set(want), mode


def test_cases_hold_the_reference_behaviours_to_keep(runs):
    L = KH.load_host()
    at_threshold = stale_matters = low_neighbour = collapse = unsorted = empty_list = 0
    for name, (case, db, res) in runs.items():
        _, res0 = KH.host_case(L, case, zero_scores=True)
        for q, r, r0 in zip(case["queries"], res, res0):
            ev = r["events"]
            # common_words == minCommonWords exactly: in the list, not scored
            hit = (r["common"] == ev["min_common"]) & (r["common"] > 0)
            at_threshold += int(hit.sum())
            assert all(KH.EXITS[e] == "word_threshold" for e in r["exits"][hit])
            # a stale mRelocScore changes pBestKF or the retained set: the result differs once the scores are zeroed on entry
            if q["mode"] == 0 and (r["n_cand"] != r0["n_cand"] or r["cand"].tolist() != r0["cand"].tolist()):
                assert ev["stale_neighbour"] > 0
                stale_matters += 1
            if q["mode"] == 1:
                low_neighbour += ev["low_neighbour"]
                empty_list += r["n_scored"] > 0 and r["n_cand"] == 0
            collapse += int((r["exits"] == KH.EXITS.index("duplicate")).sum())
            sharing = r["sharing"][:ev["n_sharing"]]
            unsorted += bool((np.diff(sharing) < 0).any())
    assert at_threshold > 0 and stale_matters > 0 and low_neighbour > 0 and collapse > 0 and unsorted > 0 and empty_list > 0


def test_fixture_shows_the_same_behaviours():
    """the same facts read from the real reference's fixture alone"""
    G = KH.golden()
    at_threshold = collapse = 0
    for name in KC.CASES:
        common, n_scored, n_cand = G[name + "_common"], G[name + "_n_scored"], G[name + "_n_cand"]
        for q in range(len(n_cand)):
            min_common = int(np.float32(common[q].max()) * np.float32(0.8))
            assert (common[q] > min_common).sum() == n_scored[q]
            at_threshold += int(((common[q] == min_common) & (common[q] > 0)).sum())
            collapse += n_cand[q] < n_scored[q]
        # the scores carry: a query's input is the previous query's output of the same mode
        assert np.array_equal(G[name + "_score_in"][1:8], G[name + "_score"][0:7]) and np.array_equal(G[name + "_score_in"][9:], G[name + "_score"][8:-1])
    assert at_threshold > 0 and collapse > 0


def test_optimised_restatement_is_the_same(runs):
    """the -O3 build tools/kfdb_bench.py times gives the same bits"""
    L3 = KH.load_host("-O3")
    for name, (case, db, res) in runs.items():
        _, res3 = KH.host_case(L3, case)
        for r, r3 in zip(res, res3):
            assert r["cand"].tolist() == r3["cand"].tolist() and r["score"].view(np.uint32).tolist() == r3["score"].view(np.uint32).tolist()
