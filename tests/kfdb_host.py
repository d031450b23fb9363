"""Helpers of the key-frame database tests (not a test module): the host restatement tests/host_shim/kfdb_host.cpp, built with g++ -ffp-contract=off and called through
ctypes, and the fixture tests/golden/kfdb_ref.npz that tools/gen_golden_kfdb.py wrote from the REAL reference."""
import ctypes
import os
import subprocess

import numpy as np

import kfdb_cases as KC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "host_shim", "libkfdb_host.so")
GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "kfdb_ref.npz")

# enum Exit / enum Event of tests/host_shim/kfdb_host.cpp
EXITS = ("not_sharing", "excluded", "word_threshold", "below_min_score", "not_retained", "duplicate", "candidate")
EVENTS = ("low_neighbour", "stale_neighbour", "best_is_neighbour", "min_common", "max_common", "n_sharing")

_HOST = {}


def golden():
    return np.load(GOLDEN_PATH)


def load_host(opt="-O2"):
    """the restatement, built on first use"""
    if opt in _HOST:
        return _HOST[opt]
    src = os.path.join(ROOT, "tests", "host_shim", "kfdb_host.cpp")
    so = SO if opt == "-O2" else SO.replace(".so", opt.replace("-", "_") + ".so")
    if not os.path.exists(so) or os.path.getmtime(src) > os.path.getmtime(so):
        subprocess.check_call(["g++", opt, "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", so, src])
    L = ctypes.CDLL(so)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.kfdb_detect_host.restype = ci
    L.kfdb_detect_host.argtypes = [ci, ci, ci, ci] + [vp] * 6 + [ci, vp, vp, vp, ctypes.c_float] + [vp] * 7
    L.bow_score_host.restype = None
    L.bow_score_host.argtypes = [ci, vp, vp, vp, ci, vp, vp, vp, ci, vp]
    _HOST[opt] = L
    return L


def host_detect(L, db, mode, q_word, q_value, excluded, min_score, score, report=True):
    """one query against the arrays of one database (KC.database_arrays) -> dict; `score` [kf_stride] f32 is the members' state on entry and is not changed"""
    S, W = db["bow_word"].shape
    score = np.array(score, np.float32)
    out = dict(score=score, common=np.zeros(S, np.int32), cand=np.full(S, -1, np.int32), exits=np.zeros(S, np.int32), sharing=np.full(S, -1, np.int32),
               events=np.zeros(len(EVENTS), np.int64))
    qw = np.ascontiguousarray(q_word, np.int32); qv = np.ascontiguousarray(q_value, np.float64)
    ex = None if excluded is None else np.ascontiguousarray(np.concatenate([excluded, np.zeros(S - len(excluded), np.uint8)]), np.uint8)
    ns = ctypes.c_int32(0)
    p = lambda a: a.ctypes.data
    out["n_cand"] = L.kfdb_detect_host(mode, int(db["n_kf"]), S, W, p(db["present"]), p(db["add_seq"]), p(db["bow_n"]), p(db["bow_word"]), p(db["bow_value"]), p(db["covis"]),
                                       len(qw), p(qw), p(qv), None if ex is None else p(ex), float(min_score), p(score), p(out["common"]), p(out["cand"]),
                                       ctypes.addressof(ns), p(out["exits"]) if report else None, p(out["sharing"]) if report else None,
                                       p(out["events"]) if report else None)
    out["n_scored"] = ns.value
    out["events"] = dict(zip(EVENTS, out["events"].tolist()))
    return out


def host_case(L, case, zero_scores=False):
    """the case's queries one after the other on the same database, mRelocScore / mLoopScore carried from query to query (or zeroed before each: zero_scores)
    -> (database arrays, [per query: the dict of host_detect + score_in])"""
    db = KC.database_arrays(case)
    state = [np.zeros(KC.KF_STRIDE, np.float32), np.zeros(KC.KF_STRIDE, np.float32)]
    res = []
    for q in case["queries"]:
        m = q["mode"]
        if zero_scores:
            state[m] = np.zeros(KC.KF_STRIDE, np.float32)
        r = host_detect(L, db, m, q["word"], q["value"], q["excluded"] if m else None, q["min_score"], state[m])
        r["score_in"] = state[m].copy()
        state[m] = r["score"].copy()
        res.append(r)
    return db, res


def host_bow_score(L, pairs_bow):
    """[(aw, av, bw, bv)] -> [P] doubles"""
    P = len(pairs_bow)
    sa = max(max(len(x[0]) for x in pairs_bow), 1); sb = max(max(len(x[2]) for x in pairs_bow), 1)
    an = np.zeros(P, np.int32); bn = np.zeros(P, np.int32)
    aw = np.zeros((P, sa), np.int32); av = np.zeros((P, sa)); bw = np.zeros((P, sb), np.int32); bv = np.zeros((P, sb))
    for p, (w1, v1, w2, v2) in enumerate(pairs_bow):
        an[p] = len(w1); aw[p, :len(w1)] = w1; av[p, :len(w1)] = v1; bn[p] = len(w2); bw[p, :len(w2)] = w2; bv[p, :len(w2)] = v2
    out = np.zeros(P)
    L.bow_score_host(P, an.ctypes.data, aw.ctypes.data, av.ctypes.data, sa, bn.ctypes.data, bw.ctypes.data, bv.ctypes.data, sb, out.ctypes.data)
    return out, (an, aw, av, sa, bn, bw, bv, sb)
