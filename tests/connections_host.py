"""Helpers of the covisibility-graph tests (not a test module): a NumPy / plain-Python restatement of KeyFrame::UpdateConnections with AddConnection and
UpdateBestCovisibles (reference src/KeyFrame.cc:298-432, :132-166) run over a case's list IN ORDER, on the unpadded cases of tests/connections_cases.py, and the
fixture tests/golden/connections_ref.npz that tools/gen_golden_connections.py wrote from the REAL reference lines."""
import os

import numpy as np

import connections_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "connections_ref.npz")
NCOVIS = 10
_gold = {}


def golden():
    if "z" not in _gold:
        _gold["z"] = np.load(GOLDEN_PATH)
    return _gold["z"]


def golden_case(name):
    """the fixture's record of a case -> (per map dict(conn_w [nk, nk], ord_kf, ord_w (nk arrays), parent, first), new_parent [L])"""
    gold, case = golden(), CC.make(name)
    states = []
    for g, M in enumerate(case["maps"]):
        n, kf, w = gold[f"{name}/{g}/ord_n"], gold[f"{name}/{g}/ord_kf"], gold[f"{name}/{g}/ord_w"]
        cut = np.concatenate([[0], np.cumsum(n)])
        conn = np.zeros((M["nk"], M["nk"]), np.int32)
        rows = gold[f"{name}/{g}/conn"]                               # (x, k, weight) of every stored weight
        conn[rows[:, 0], rows[:, 1]] = rows[:, 2]
        states.append(dict(conn_w=conn, ord_kf=[kf[cut[k]:cut[k + 1]] for k in range(M["nk"])], ord_w=[w[cut[k]:cut[k + 1]] for k in range(M["nk"])],
                           parent=gold[f"{name}/{g}/parent"], first=gold[f"{name}/{g}/first"]))
    return states, gold[f"{name}/new_parent"]


def read_driver_output(case, r):
    """the int32 record the fixture's driver and tests/adapter_shim/adapter_connections_main.cpp write -> (states, new_parent) as golden_case gives them"""
    at = 0

    def take(n):
        nonlocal at
        v = r[at:at + n]; at += n
        assert len(v) == n
        return v
    states = []
    for M in case["maps"]:
        nk = M["nk"]
        st = dict(conn_w=np.zeros((nk, nk), np.int32), ord_kf=[], ord_w=[], parent=np.zeros(nk, np.int32), first=np.zeros(nk, np.uint8))
        for k in range(nk):
            row = take(2 * int(take(1)[0])).reshape(-1, 2)
            st["conn_w"][k, row[:, 0]] = row[:, 1]
            n = int(take(1)[0]); st["ord_kf"].append(take(n)); st["ord_w"].append(take(n))
            st["parent"][k], st["first"][k] = take(2)
            take(int(take(1)[0]))                                      # the children added
        states.append(st)
    new_parent = take(len(case["entries"]))
    assert at == len(r)
    return states, new_parent


def _update_best(M, st, x):
    row = st["conn_w"][x]
    pairs = sorted((int(row[k]), int(M["kf_rank"][k]), int(k)) for k in np.flatnonzero(row > 0))
    st["ord_kf"][x] = [k for _, _, k in reversed(pairs)]; st["ord_w"][x] = [w for w, _, _ in reversed(pairs)]


def _add_connection(M, st, x, j, w):
    if st["conn_w"][x, j] == w:
        return
    st["conn_w"][x, j] = w
    _update_best(M, st, x)


def host_case(case):
    """-> (per map the state after the list: dict(conn_w, ord_kf, ord_w, parent, first), new_parent [L], status [L])"""
    states = [dict(conn_w=M["conn_w"].copy(), ord_kf=[list(map(int, o)) for o in M["ord_kf"]], ord_w=[list(map(int, o)) for o in M["ord_w"]], parent=M["parent"].copy(),
                   first=M["first"].copy()) for M in case["maps"]]
    L = len(case["entries"])
    new_parent, status = np.full(L, -1, np.int32), np.zeros(L, np.int32)
    for l, (g, j) in enumerate(case["entries"]):
        M, st = case["maps"][g], states[g]
        counter = np.zeros(M["nk"], np.int64)
        for p in M["pts"][j]:
            if p >= 0 and not M["pt_bad"][p]:
                np.add.at(counter, np.asarray(M["obs"][p], np.int64), 1)
        counter[j] = 0
        if not counter.any():
            status[l] = 1
            continue
        nmax, kmax, pairs = 0, -1, []
        for k in sorted(np.flatnonzero(counter), key=lambda k: M["kf_rank"][k]):
            c = int(counter[k])
            if c > nmax:
                nmax, kmax = c, int(k)
            if c >= CC.TH:
                pairs.append((c, int(M["kf_rank"][k]), int(k)))
                _add_connection(M, st, k, j, c)
        if not pairs:
            pairs.append((nmax, int(M["kf_rank"][kmax]), kmax))
            _add_connection(M, st, kmax, j, nmax)
        pairs.sort()
        st["conn_w"][j] = counter
        st["ord_kf"][j] = [k for _, _, k in reversed(pairs)]; st["ord_w"][j] = [w for w, _, _ in reversed(pairs)]
        if st["first"][j] and M["mnid"][j] != 0:
            st["parent"][j] = st["ord_kf"][j][0]
            st["first"][j] = 0
            new_parent[l] = st["ord_kf"][j][0]
    return states, new_parent, status


def covis_of(st):
    """the first ten of every ordered list, padded with -1"""
    out = np.full((len(st["ord_kf"]), NCOVIS), -1, np.int32)
    for k, o in enumerate(st["ord_kf"]):
        out[k, :min(len(o), NCOVIS)] = np.asarray(o[:NCOVIS], np.int32)
    return out


def assert_state_equal(got, want, where=""):
    """exact equality of two per-map states (conn_w, ordered lists with weights, parent, first)"""
    np.testing.assert_array_equal(got["conn_w"], want["conn_w"], err_msg=f"{where} conn_w")
    np.testing.assert_array_equal(got["parent"], want["parent"], err_msg=f"{where} parent")
    np.testing.assert_array_equal(np.asarray(got["first"]) != 0, np.asarray(want["first"]) != 0, err_msg=f"{where} first")
    assert len(got["ord_kf"]) == len(want["ord_kf"])
    for k in range(len(want["ord_kf"])):
        np.testing.assert_array_equal(np.asarray(got["ord_kf"][k], np.int32), np.asarray(want["ord_kf"][k], np.int32), err_msg=f"{where} ord_kf[{k}]")
        np.testing.assert_array_equal(np.asarray(got["ord_w"][k], np.int32), np.asarray(want["ord_w"][k], np.int32), err_msg=f"{where} ord_w[{k}]")
