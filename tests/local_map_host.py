"""Helpers of the local-map tests (not a test module): a NumPy / plain-Python restatement of Tracking::UpdateLocalMap (reference src/Tracking.cc:2394-2552) with the
head loops of SearchLocalPoints / SearchLocalLines (:2289-2312, :2334-2358) on the unpadded cases of tests/local_map_cases.py, and the fixture
tests/golden/local_map_ref.npz that tools/gen_golden_local_map.py wrote from the REAL reference lines."""
import os

import numpy as np

import local_map_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "local_map_ref.npz")
KEYS = ("local_kf", "ref_kf", "lp", "lp_seen", "ll", "ll_seen", "match", "line_match")    # what the reference leaves behind; the status is the restatement's


def golden():
    return np.load(GOLDEN_PATH)


def golden_frame(gold, name, f):
    """the fixture's record of frame f of a case -> dict of int arrays (ref_kf as an int)"""
    r = {k: gold[f"{name}/{f}/{k}"] for k in KEYS}
    r["ref_kf"] = int(r["ref_kf"])
    return r


def first_occurrences(local_kf, slots, bad):
    """UpdateLocalPoints / UpdateLocalLines: the ids of the local key frames' slots in order, each once, NULL and bad ones left out"""
    seen, out = set(), []
    for k in local_kf:
        for i in slots[k]:
            i = int(i)
            if i < 0 or i in seen:
                continue
            if not bad[i]:
                out.append(i)
                seen.add(i)
    return out


def host_frame(case, f):
    """frame f of a case -> the dict the fixture holds"""
    F = case["frames"][f]; M = case["maps"][F["map"]]
    match, line_match = F["match"].copy(), F["line_match"].copy()
    counter = {}
    for i, p in enumerate(match):
        if p >= 0:
            if M["pt_bad"][p]:
                match[i] = -1
            else:
                for k in M["obs"][p]:
                    counter[k] = counter.get(k, 0) + 1
    local, ref, status = list(F["local_in"]), -1, 1
    if counter:
        status, local, mark, best = 0, [], set(), 0
        for k in sorted(counter, key=lambda k: M["kf_rank"][k]):
            if M["kf_bad"][k]:
                continue
            if counter[k] > best:
                best, ref = counter[k], k
            local.append(k); mark.add(k)
        for it in range(len(local)):
            if len(local) > 80:
                break
            k = local[it]
            for n in M["covis"][k]:
                if n >= 0 and not M["kf_bad"][n] and n not in mark:
                    local.append(int(n)); mark.add(int(n))
                    break
            for c in M["children"][k]:
                if not M["kf_bad"][c] and c not in mark:
                    local.append(int(c)); mark.add(int(c))
                    break
            pa = int(M["parent"][k])
            if pa >= 0 and pa not in mark:
                local.append(pa); mark.add(pa)
                break
    for i, l in enumerate(line_match):
        if l >= 0 and M["ml_bad"][l]:
            line_match[i] = -1
    lp = first_occurrences(local, M["pts"], M["pt_bad"])
    ll = first_occurrences(local, M["lines"], M["ml_bad"])
    held, lheld = set(int(p) for p in match if p >= 0), set(int(l) for l in line_match if l >= 0)
    a = lambda x: np.asarray(x, np.int32)
    return dict(local_kf=a(local), ref_kf=int(ref), lp=a(lp), lp_seen=a([p in held for p in lp]), ll=a(ll), ll_seen=a([l in lheld for l in ll]), match=a(match),
                line_match=a(line_match), status=status)


def out_strides(case, gold):
    """(lp_stride, ll_stride) of a case's call: beyond the longest list, or one below it for a `short` case"""
    n_lp = [len(gold[f"{case['name']}/{f}/lp"]) for f in range(len(case["frames"]))]
    n_ll = [len(gold[f"{case['name']}/{f}/ll"]) for f in range(len(case["frames"]))]
    if case["short"]:
        return max(n_lp) - 1, max(n_ll) - 1
    return max(n_lp) + 3, max(n_ll) + 2
