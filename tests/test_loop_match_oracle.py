"""CPU: the sequential restatement tests/host_shim/loop_match_host.cpp equals the fixture the REAL reference wrote (tests/golden/loop_match_ref.npz, from
src/ORBmatcher.cc compiled where it lies by tools/gen_golden_loop_match.py) for every case of the four loop-closing matchers, bit for bit; over the fixture cases
every exit of every function is reached; and every fixture case has at least 30 accepted matches per function, so a kernel that returns nothing cannot pass."""
import numpy as np
import pytest

import loop_match_cases as LC


@pytest.fixture(scope="module")
def host():
    return LC.load_host()


@pytest.fixture(scope="module")
def G():
    return np.load(LC.GOLDEN_PATH)


@pytest.fixture(scope="module")
def sim3(host):
    return {name: (LC.sim3_case(**args), th) for name, args, th in LC.SIM3_CASES}


def count(exits, names):
    return {names[k]: int((exits == k).sum()) for k in range(len(names))}


def test_sim3_restatement_equals_the_reference_and_reaches_every_exit(host, G, sim3):
    reached = [dict.fromkeys(LC.SIM3_EXITS, 0), dict.fromkeys(LC.SIM3_EXITS, 0)]
    events = dict.fromkeys(LC.SIM3_EVENTS, 0)
    scales = set()
    for name, (case, th) in sim3.items():
        m, nf, e1, e2, ev = LC.host_sim3(host, case, th)
        assert np.array_equal(nf, G[name + "_n_found"]), name
        assert np.array_equal(m, G[name + "_match12"].astype(np.int32)), name
        assert nf.sum() >= 30, name
        # what is accepted is exactly what changed, and nothing that held a match on entry changed
        changed = m != case["match12"]
        assert changed.sum() == nf.sum() and (case["match12"][changed] == -1).all()
        assert (e1 == LC.SIM3_EXITS.index("accepted")).sum() == nf.sum() == (e2 == LC.SIM3_EXITS.index("accepted")).sum()
        for d, e in enumerate((e1, e2)):
            for k, v in count(e, LC.SIM3_EXITS).items():
                reached[d][k] += v
        for k, v in ev.items():
            events[k] += v
        scales |= {("below" if s < 1 else "above" if s > 1 else "one") for s in case["s12"].tolist()}
    print(reached, events)
    for d in (0, 1):                                            # in each direction
        missing = [k for k, v in reached[d].items() if v == 0]
        assert not missing, (d, missing)
    assert all(v > 0 for v in events.values()), events         # an entry index outside [0, N2), the level gate removing the nearest descriptor, a Hamming tie
    assert scales == {"below", "one", "above"}


def test_bow_restatement_equals_the_reference_and_reaches_every_exit(host, G):
    reached = dict.fromkeys(LC.BOW_EXITS, 0)
    events = dict.fromkeys(LC.BOW_EVENTS, 0)
    for name, args, nn_ratio, ori in LC.BOW_CASES:
        case = LC.bow_case(**args)
        m, nm, ex, ev = LC.host_bow(host, case, nn_ratio, ori)
        assert np.array_equal(nm, G[name + "_nmatches"]), name
        assert np.array_equal(m, G[name + "_match12"].astype(np.int32)), name
        assert nm.sum() >= 30 and (m >= 0).sum() == nm.sum(), name
        for k, v in count(ex, LC.BOW_EXITS).items():
            reached[k] += v
        for k, v in ev.items():
            events[k] += v
    print(reached, events)
    assert all(v > 0 for v in reached.values()), reached
    # bestDist1 == 50 rejected (it ends in dist_rejected: the test is strict), an idx1 whose best idx2 an earlier idx1 took, a node present in key frame 2 only
    assert all(v > 0 for v in events.values()), events


@pytest.fixture(scope="module")
def scw():
    return {name: (LC.scw_case(**args), th, fth) for name, args, th, fth in LC.SCW_CASES}


PROJ_EXITS = LC.SCW_EXITS[:LC.SCW_EXITS.index("accepted") + 1]
FUSE_EXITS = tuple(k for k in LC.SCW_EXITS if k not in ("found", "all_blocked", "accepted"))     # "found" is part of `usable` there; nothing blocks a fuse candidate


def test_projection_scw_restatement_equals_the_reference_and_reaches_every_exit(host, G, scw):
    reached = dict.fromkeys(PROJ_EXITS, 0)
    events = dict.fromkeys(LC.SCW_EVENTS[:3], 0)
    for name, (case, th, _) in scw.items():
        m, nm, ex, ev = LC.host_projection_scw(host, case, th)
        assert np.array_equal(nm, G[name + "_nmatches"]), name
        assert np.array_equal(m, G[name + "_kf_match"].astype(np.int32)), name
        assert nm.min() >= 20 and nm.sum() >= 30 and (m >= 0).sum() == nm.sum(), name
        assert not (m[case["kf"]["blocked"] != 0] >= 0).any()                          # a key point matched on entry is never written
        for k in PROJ_EXITS:
            reached[k] += int((ex == LC.SCW_EXITS.index(k)).sum())
        for k in events:
            events[k] += ev[k]
    print(reached, events)
    assert all(v > 0 for v in reached.values()), reached
    assert all(v > 0 for v in events.values()), events         # bestDist == 50 accepted, blocked on entry, taken earlier in this call so that the result changes


def test_fuse_scw_restatement_equals_the_reference_and_reaches_every_exit(host, G, scw):
    reached = dict.fromkeys(FUSE_EXITS, 0)
    most = 0
    for name, (case, _, th) in scw.items():
        fi, ow, nf, ex, ev = LC.host_fuse_scw(host, case, th)
        assert np.array_equal(nf, G[name + "_n_fused"]), name
        assert np.array_equal(fi, G[name + "_fuse_idx"].astype(np.int32)), name
        assert np.array_equal(ow, G[name + "_owner"].astype(np.int32)), name
        assert nf.min() >= 30 and (fi >= 0).sum() == nf.sum(), name
        # the key frame's slots after the call, as the reference left them: the owner of every empty slot that was chosen
        slots = np.full(case["kf"]["keys_un"].shape, -1, np.int32)
        for b, j in zip(*np.nonzero((fi >= 0) & (ow == np.arange(ow.shape[1])[None, :]))):
            slots[b, fi[b, j]] = j
        assert np.array_equal(slots, G[name + "_slots"].astype(np.int32)), name
        for k in FUSE_EXITS:
            reached[k] += int((ex == LC.SCW_EXITS.index(k)).sum())
        most = max(most, ev["max_points_on_one_slot"])
    print(reached, most)
    assert all(v > 0 for v in reached.values()), reached       # every gate and each of the four outcomes of `owner`
    assert most >= 3                                            # three points on one slot
