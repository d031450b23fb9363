"""GPU parity (bit-exact) of the order-bound pass of planarslam_amd/csrc/guided.hip, the speculating resolver (a thread per probe, rounds that commit up to the first
conflict) and its wave-wide fallback, against oracle_lib.search_by_projection_frame / search_by_projection_map on inputs built to stress it
(tests/spec_resolve_cases.py).  Every case first asserts on its inputs, in numpy, the share of probes whose window holds a key point that also lies in the window of
an earlier probe of the same 256-probe chunk (spec_resolve_cases.shared_share).  Shares measured on the generators, per frame:

    crowded(N=300, crowd=0.7, dup=0.9), th = 15                    frame: 0.81 0.82 0.87 (mixed and all-observed alike; lists up to 17)
    crowded_map(N=300, crowd=0.7, 700 probes), th = 1 / 3          map:   0.30 0.31 0.40 / 0.58 0.54 0.60 (lists up to 4 / 13)
    ... with one level everywhere, th = 1 / 3                      map:   0.41 0.39 0.47 / 0.69 0.66 0.73 (lists up to 6 / 24)
    one_shared_candidate(300 probes)                                0.993 = all but the first probe of each chunk; every list is [key point 0]
    no_shared_candidate (165 probes)                                0
    cluster(64) / cluster(65) / cluster(48, 400 probes), th = 3     0.995; every list holds the 64 / 65 / 48 key points of the cluster
"""
import numpy as np
import pytest

import oracle_lib as O
import spec_resolve_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from planarslam_amd._lib import Context
    return Context(0)


def frame_parity(ctx, cur, last, th, ori, cur_match=None):
    from planarslam_amd.guided import ORBmatcher
    ref_m, ref_n = O.search_by_projection_frame(cur, last, th, check_orientation=ori, cur_match=cur_match)
    m, n = ORBmatcher(0.9, ori, ctx).SearchByProjectionFrame(cur, last, th, cur_match=cur_match)
    np.testing.assert_array_equal(n, ref_n)
    np.testing.assert_array_equal(m, ref_m)
    return m, n


def map_parity(ctx, fr, pr, th, ratio, match=None):
    from planarslam_amd.guided import ORBmatcher
    ref_m, ref_n = O.search_by_projection_map(fr, pr, th=th, nn_ratio=ratio, match=match)
    m, n = ORBmatcher(ratio, True, ctx).SearchByProjectionMap(fr, pr, th=th, match=match)
    np.testing.assert_array_equal(n, ref_n)
    np.testing.assert_array_equal(m, ref_m)
    return m, n


@pytest.mark.parametrize("all_observed", [False, True])
@pytest.mark.parametrize("ori", [True, False])
def test_frame_conflict_heavy(ctx, all_observed, ori):
    cur, last = K.crowded(all_observed=all_observed)
    for b in range(3):
        assert K.shared_share(K.frame_windows(cur, last, b, 15.0)) >= 0.25
    assert all_observed == bool(last["mp_observed"].all())
    m, n = frame_parity(ctx, cur, last, 15.0, ori)
    assert n.min() > 10          # dup = 0.9: the last frame's map points stem from a tenth of the key points


@pytest.mark.parametrize("all_observed", [False, True])
@pytest.mark.parametrize("equal_levels", [False, True])
def test_map_conflict_heavy_both_ratios(ctx, all_observed, equal_levels):
    """nn_ratio 0.6 and 0.8; with one level everywhere the ratio test always applies, with the generator's levels best and second best often differ in level"""
    fr, pr = K.crowded_map(all_observed=all_observed, equal_levels=equal_levels)
    for th in (1.0, 3.0):
        for b in range(3):
            assert K.shared_share(K.map_windows(fr, pr, b, th)) >= 0.25
        got = [map_parity(ctx, fr, pr, th, ratio) for ratio in (0.6, 0.8)]
        assert got[0][1].min() > 20
    assert (got[0][1] != got[1][1]).any()      # at th = 3 the ratio test decides some probes


@pytest.mark.parametrize("observed", [None, 0, 1])
def test_every_probe_shares_one_candidate(ctx, observed):
    """one commit per round: observed probes leave the key point blocked for the rest, unobserved ones take it one after another"""
    fr, pr = K.one_shared_candidate(observed=observed)
    w = K.map_windows(fr, pr, 0, 1.0)
    assert all(list(x) == [0] for x in w) and K.shared_share(w) >= 0.99
    m, n = map_parity(ctx, fr, pr, 1.0, 0.8)
    assert m[0, 0] >= 0 and (m[0, 1:] == -1).all()


def test_no_shared_candidate(ctx):
    """one round per chunk"""
    fr, pr = K.no_shared_candidate()
    w = K.map_windows(fr, pr, 0, 1.0)
    assert K.shared_share(w) == 0 and all(len(x) == 1 for x in w)
    m, n = map_parity(ctx, fr, pr, 1.0, 0.8)
    assert n[0] == len(w)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 255, 256, 257])
def test_probe_counts(ctx, count):
    cur, last = K.crowded()
    last["n"][:] = np.minimum(last["n"], count)
    assert last["n"][0] == count
    if count >= 63:
        assert K.shared_share(K.frame_windows(cur, last, 0, 15.0)) >= 0.25
    frame_parity(ctx, cur, last, 15.0, True)
    fr, pr = K.crowded_map()
    pr["n"][:] = count
    if count >= 63:
        assert K.shared_share(K.map_windows(fr, pr, 0, 3.0)) >= 0.25
    map_parity(ctx, fr, pr, 3.0, 0.8)


@pytest.mark.parametrize("n_in", [K.SPEC_MAX_LIST, K.SPEC_MAX_LIST + 1])
@pytest.mark.parametrize("observed", [None, 1])
def test_lists_at_the_fallback_threshold_and_one_above(ctx, n_in, observed):
    fr, pr = K.cluster(n_in, observed=observed)
    w = K.map_windows(fr, pr, 0, 3.0)
    assert all(len(x) == n_in for x in w) and K.shared_share(w) >= 0.25
    m, n = map_parity(ctx, fr, pr, 3.0, 0.8)
    assert n[0] > 10


def test_chunks_cut_by_the_candidate_capacity(ctx):
    """48-entry lists: 256 probes would need 12 288 list entries, so the chunks are cut at 170 probes"""
    fr, pr = K.cluster(48, P=400, extra=100)
    w = K.map_windows(fr, pr, 0, 3.0)
    assert sum(len(x) for x in w[:K.CHUNK]) > K.CAND_CAP and max(len(x) for x in w) <= K.SPEC_MAX_LIST and K.shared_share(w) >= 0.25
    map_parity(ctx, fr, pr, 3.0, 0.8)


def test_initial_blocked_mask_and_matches(ctx):
    rng = np.random.default_rng(77)
    cur, last = K.crowded()
    cur["blocked"] = (rng.random(cur["blocked"].shape) < 0.3).astype(np.uint8)
    init = rng.integers(-1, 500, cur["blocked"].shape).astype(np.int32)
    assert K.shared_share(K.frame_windows(cur, last, 0, 15.0)) >= 0.25
    m, n = frame_parity(ctx, cur, last, 15.0, True, cur_match=init)
    assert (m == init).any() and (m != init).any()
    fr, pr = K.crowded_map()
    fr["blocked"] = (rng.random(fr["blocked"].shape) < 0.3).astype(np.uint8)
    assert K.shared_share(K.map_windows(fr, pr, 0, 3.0)) >= 0.25
    m, n = map_parity(ctx, fr, pr, 3.0, 0.8, match=init)
    assert (m == init).any() and (m != init).any()


@pytest.mark.parametrize("n_in", [12, K.SPEC_MAX_LIST + 6])
def test_exact_distance_ties_take_the_first_in_list_order(ctx, n_in):
    """identical descriptors: every distance is 0, both resolvers must take the first unblocked entry of the list, and the ratio test (0 > ratio * 0) never fails"""
    fr, pr = K.cluster(n_in, P=100, same_desc=True)
    w = K.map_windows(fr, pr, 0, 3.0)
    assert all(len(x) == n_in for x in w) and K.shared_share(w) >= 0.25
    assert (fr["desc"][0] == fr["desc"][0, 0]).all() and (pr["desc"][0] == fr["desc"][0, 0]).all()
    m, n = map_parity(ctx, fr, pr, 3.0, 0.6)
    assert n[0] >= 1
