"""CPU: the plain C++ restatement of LocalMapping::CreateNewMapLines2 and its searches (tests/host_shim/new_lines_host.cpp) against the fixture the REAL reference
wrote (tests/golden/new_lines_ref.npz, tools/gen_golden_new_lines.py): matches, thresholds and the six floats of every line bit for bit, and the conditions that make
the fixture mean something.  The exit report of the restatement must reach every exit over all cases; the ones it cannot reach are named in UNREACHED."""
import numpy as np
import pytest

import new_lines_cases as LC
from new_lines_host import EVENTS, EXITS, golden, golden_create, host_average_dir, host_create, host_search, load_host, neighbour0

# dist_zero: an end point exactly on a camera centre in float needs a non-finite or hand-made pose (expected by the issue).
UNREACHED = {"dist_zero"}


@pytest.fixture(scope="module")
def host():
    return load_host()


@pytest.fixture(scope="module")
def G():
    return golden()


@pytest.fixture(scope="module")
def runs(host):
    out = {}
    for name, args in LC.CASES + LC.HOST_CASES:
        cam, cur, neigh, nn = LC.new_lines_case(**args)
        out[name] = (args, cur, neigh) + host_create(host, cam, cur, neigh, nn, args["K"])
    return out


@pytest.mark.parametrize("case", LC.CASES, ids=[c[0] for c in LC.CASES])
def test_restatement_equals_the_reference(runs, G, case):
    name = case[0]
    got, ref = runs[name][3], golden_create(G, name)
    np.testing.assert_array_equal(got[0], ref[0])
    for a, b in zip(got[1:4], ref[1:4]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(got[4].view(np.uint64), ref[4].view(np.uint64))
    assert got[0].min() > 0
    # the six values are floats widened to double
    assert np.array_equal(got[4], got[4].astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("case", LC.CASES, ids=[c[0] for c in LC.CASES])
def test_searches_equal_the_reference(host, runs, G, case):
    name, args = case
    cur, neigh = runs[name][1], runs[name][2]
    m, nm, a, b = host_search(host, cur, neighbour0(neigh, args["K"]), 0)
    np.testing.assert_array_equal(m, G[name + "_tri_match"]); np.testing.assert_array_equal(nm, G[name + "_tri_n"])
    np.testing.assert_array_equal(np.stack([a, b], 1).view(np.uint64), G[name + "_mads"].view(np.uint64))
    assert nm.min() > 0 and (G[name + "_mads"] > 0).all()
    m, nm, _, _ = host_search(host, cur, neighbour0(neigh, args["K"]), 1)
    np.testing.assert_array_equal(m, G[name + "_desc_match"]); np.testing.assert_array_equal(nm, G[name + "_desc_n"])
    assert nm.sum() > 0


def test_update_average_dir_equals_the_reference(host, G):
    d = LC.average_dir_case()
    nrm, mn, mx = host_average_dir(host, d)
    np.testing.assert_array_equal(nrm.view(np.uint64), G["dir_normal"].view(np.uint64))
    np.testing.assert_array_equal(mn.view(np.uint32), G["dir_min"].view(np.uint32)); np.testing.assert_array_equal(mx.view(np.uint32), G["dir_max"].view(np.uint32))
    assert (mx[0] > mn[0]).all() and np.abs(np.linalg.norm(nrm[0], axis=1) - 1).max() < 0.2


def test_the_fixture_cases_mean_something(runs):
    """per reference-made case: what the occupancy rule, the stereo sources and the baseline gate decide"""
    ex = {n: np.bincount(runs[n][4].ravel(), minlength=len(EXITS)) for n in runs}
    ev = {n: dict(zip(EVENTS, runs[n][5].tolist())) for n in runs}
    ref = [c[0] for c in LC.CASES]
    for n in ref:
        args, cur, neigh = runs[n][:3]
        K = args["K"]
        assert all(neigh["n"][b * K + k] <= cur["n"][b] for b in range(len(cur["n"])) for k in range(K))   # the reference never reads past mvDepthLine
        assert ev[n]["idx2_past_n1"] == 0
        assert ev[n]["rejected_then_accepted"] > 0, n            # accepted at k > 0 after a pair of it was rejected by a gate at an earlier neighbour
        assert ex[n][EXITS.index("taken_would_survive")] > 0, n  # a later pair of an accepted idx1 survives every gate: the occupancy rule decides
        assert ev[n]["shared_idx2"] > 0, n                       # one idx2 taken by two lines
        assert ev[n]["src_stereo1"] > 0 and ev[n]["src_stereo2"] > 0, n
        got = runs[n][3]
        assert (np.diff(got[1][0, :got[0][0]]) >= 0).all()        # creation order: k ascending
    assert ex["small"][EXITS.index("neigh_baseline")] > 0        # one neighbour fails the baseline gate
    assert ev["past_n1"]["idx2_past_n1"] > 0                      # restatement only: the documented "not stereo" rule


def test_every_exit_is_reached(host, runs):
    total = sum(np.bincount(runs[n][4].ravel(), minlength=len(EXITS)) for n in runs)
    # a neighbour with one line (lmatches[i][1] does not exist): restatement only
    args = LC.CASES[0][1]
    cam, cur, neigh, nn = LC.new_lines_case(**args)
    neigh["n"] = neigh["n"].copy(); neigh["n"][0] = 1
    _, exits, _ = host_create(host, cam, cur, neigh, nn, args["K"])
    total = total + np.bincount(exits.ravel(), minlength=len(EXITS))
    missing = {EXITS[i] for i in range(1, len(EXITS)) if total[i] == 0}
    print({EXITS[i]: int(total[i]) for i in range(len(EXITS))})
    assert missing == UNREACHED
