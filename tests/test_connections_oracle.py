"""CPU test: the restatement of KeyFrame::UpdateConnections in tests/connections_host.py equals tests/golden/connections_ref.npz, what the REAL reference lines
left behind (tools/gen_golden_connections.py), on every case of tests/connections_cases.py - and each case holds what its name promises, asserted from the fixture."""
import numpy as np
import pytest

import connections_cases as CC
import connections_host as CH

TH = CC.TH


@pytest.mark.parametrize("name", CC.NAMES)
def test_restatement_equals_the_reference(name):
    case = CC.make(name)
    states, new_parent, status = CH.host_case(case)
    want, want_parent = CH.golden_case(name)
    assert len(states) == len(want)
    for g in range(len(want)):
        CH.assert_state_equal(states[g], want[g], f"{name} map {g}")
    assert np.array_equal(new_parent, want_parent)
    assert status.tolist() == ([1, 0] if name == "empty" else [0] * len(case["entries"]))


def test_fixture_holds_every_case_and_nothing_else():
    assert sorted({k.split("/")[0] for k in CH.golden().files}) == sorted(CC.NAMES)


def rank_of(M, ks):
    return [int(M["kf_rank"][k]) for k in ks]


def test_pair():
    (st,), new_parent = CH.golden_case("pair")
    assert st["conn_w"].tolist() == [[0, 20], [20, 0]]
    assert [list(o) for o in st["ord_kf"]] == [[1], [0]] and [list(o) for o in st["ord_w"]] == [[20], [20]]
    assert st["parent"].tolist() == [-1, 0] and st["first"].tolist() == [1, 0] and new_parent.tolist() == [0]


def test_threshold():
    case = CC.make("threshold")
    (st,), _ = CH.golden_case("threshold")
    assert sorted(case["counts"].values()) == [TH - 1, TH, TH + 1]
    assert st["conn_w"][0].tolist() == [0, TH - 1, TH, TH + 1]                     # the own row is the whole counter
    assert list(st["ord_kf"][0]) == [3, 2] and list(st["ord_w"][0]) == [TH + 1, TH]  # the own list holds the targets only
    assert st["conn_w"][1].sum() == 0 and len(st["ord_kf"][1]) == 0              # 14: no AddConnection
    assert st["conn_w"][2, 0] == TH and st["conn_w"][3, 0] == TH + 1


def test_fallback_max():
    case = CC.make("fallback_max")
    M = case["maps"][0]
    (st,), _ = CH.golden_case("fallback_max")
    assert max(case["counts"].values()) < TH and not np.array_equal(M["kf_rank"], np.arange(M["nk"]))
    top = [k for k, c in case["counts"].items() if c == max(case["counts"].values())]
    assert len(top) == 2
    winner = min(top, key=lambda k: M["kf_rank"][k])                            # `>` from 0 in pointer order: the first of the equal maxima
    assert list(st["ord_kf"][0]) == [winner] and list(st["ord_w"][0]) == [9]
    assert st["conn_w"][:, 0].tolist() == [9 if k == winner else 0 for k in range(M["nk"])]
    assert (st["conn_w"][0] > 0).sum() == len(case["counts"])


def test_ties():
    case = CC.make("ties")
    M = case["maps"][0]
    (st,), _ = CH.golden_case("ties")
    ws, ks = list(st["ord_w"][0]), list(st["ord_kf"][0])
    assert ws == sorted(case["counts"].values(), reverse=True) and len(set(ws)) < len(ws) and min(ws) >= TH
    for a, b in zip(range(len(ks) - 1), range(1, len(ks))):
        if ws[a] == ws[b]:
            assert M["kf_rank"][ks[a]] > M["kf_rank"][ks[b]]                    # equal weights: DESCENDING pointer order
    assert any(ws[i] == ws[i + 1] and ks[i] < ks[i + 1] for i in range(len(ks) - 1))   # the order is by rank, not by id


def test_asymmetric():
    case = CC.make("asymmetric")
    M, j = case["maps"][0], case["j"]
    (st,), _ = CH.golden_case("asymmetric")
    slots = M["pts"][j]
    good = slots[slots >= 0]
    assert (slots == -1).sum() == 7 and len(np.unique(good)) == len(good) - 1                       # NULL slots and one point held twice
    assert M["pt_bad"][good].sum() == 6
    assert sum(j not in M["obs"][p] for p in good) == TH and sum(j in M["obs"][p] for p in good) > 0  # lists without j, and self observations
    assert st["conn_w"][j].tolist() == [case["counts"].get(k, 0) for k in range(M["nk"])] and st["conn_w"][j, j] == 0
    assert sorted(st["ord_kf"][j]) == sorted(k for k, c in case["counts"].items() if c >= TH)
    assert st["conn_w"][1, j] == TH and st["conn_w"][2, j] == TH and st["conn_w"][3, j] == 0


def test_sequence():
    case = CC.make("sequence")
    n = case["names"]
    A, B, C, D, E, F, U, Z, Y = (n[k] for k in "ABCDEFUZY")
    M = case["maps"][0]
    assert [kf for _, kf in case["entries"]] == [A, D, B, C, E] and len(case["entries"]) == 5
    (st,), new_parent = CH.golden_case("sequence")
    # B came after A and counted A once more than A counted B: A's row changed and its list is ALL of its row, the sub-threshold C included
    assert st["conn_w"][A, B] == 21 and st["conn_w"][B, A] == 21
    assert list(st["ord_kf"][A]) == [B, U, C] and list(st["ord_w"][A]) == [21, 16, 5]
    # E came after D with the weight D already had: D's list is still its targets only, although its row holds F
    assert st["conn_w"][D, E] == 18 and st["conn_w"][E, D] == 18 and st["conn_w"][D, F] == 4
    assert list(st["ord_kf"][D]) == [E]
    # C's only candidate is A, below the threshold, with the weight A already had: no re-sort there either (A's list was settled by B)
    assert st["conn_w"][C].tolist() == [5 if k == A else 0 for k in range(M["nk"])] and list(st["ord_kf"][C]) == [A]
    # U is not listed: its stale weight for A is overridden, the rest of the row stays, and the list is the whole row, ties in descending pointer order
    assert st["conn_w"][U, A] == 16 and st["conn_w"][U, Z] == 9 and st["conn_w"][U, Y] == 9
    assert list(st["ord_kf"][U]) == [A] + sorted([Z, Y], key=lambda k: -M["kf_rank"][k]) and list(st["ord_w"][U]) == [16, 9, 9]
    # B is listed: its stale row vanished, and it keeps the parent it had
    assert st["conn_w"][B, F] == 0 and list(st["ord_kf"][B]) == [A] and st["parent"][B] == F and new_parent[2] == -1
    assert new_parent.tolist() == [-1, E, -1, A, D]


def test_parents():
    case = CC.make("parents")
    n = case["names"]
    M = case["maps"][0]
    (st,), new_parent = CH.golden_case("parents")
    assert M["mnid"][n["zero"]] == 0 and M["first"][n["zero"]] == 1
    assert st["parent"][n["zero"]] == -1 and st["first"][n["zero"]] == 1                       # mnId 0 never gets a parent
    assert st["ord_kf"][n["old"]][0] == n["p_new"] and st["parent"][n["old"]] == n["p_old"]    # connected before: the parent stays
    assert st["parent"][n["new"]] == n["p_new"] and st["first"][n["new"]] == 0
    assert new_parent.tolist() == [-1, -1, n["p_new"]]


def test_empty():
    case = CC.make("empty")
    M = case["maps"][0]
    (st,), new_parent = CH.golden_case("empty")
    _, _, status = CH.host_case(case)
    assert status.tolist() == [1, 0] and new_parent[0] == -1
    assert np.array_equal(st["conn_w"][0], M["conn_w"][0]) and list(st["ord_kf"][0]) == list(M["ord_kf"][0]) and list(st["ord_w"][0]) == list(M["ord_w"][0])
    assert st["parent"][0] == M["parent"][0] and st["first"][0] == 1


def test_two_maps():
    case = CC.make("two_maps")
    maps_in_order = [g for g, _ in case["entries"]]
    assert sorted(set(maps_in_order)) == [0, 1] and any(a != b for a, b in zip(maps_in_order, maps_in_order[1:]))
    assert case["maps"][0]["nk"] != case["maps"][1]["nk"]
    states, _ = CH.golden_case("two_maps")
    for g, st in enumerate(states):                                          # each map on its own gives the same
        own = dict(maps=[case["maps"][g]], entries=[(0, kf) for gg, kf in case["entries"] if gg == g])
        (alone,), _, _ = CH.host_case(own)
        CH.assert_state_equal(alone, st, f"map {g} alone")


def test_wide():
    case = CC.make("wide")
    M, hub = case["maps"][0], case["hub"]
    (st,), _ = CH.golden_case("wide")
    assert M["nk"] == 1024 and len(M["pts"][hub]) == 2000 and all(len(o) == 40 for o in M["obs"])
    assert (np.delete(st["conn_w"][hub], hub) > 0).all() and st["conn_w"][hub, hub] == 0          # connected to all 1023
    n_targets = int((case["counts"] >= TH).sum())
    assert len(st["ord_kf"][hub]) == n_targets and 512 < n_targets < 1023
    assert (st["conn_w"][:, hub] > 0).sum() == n_targets
