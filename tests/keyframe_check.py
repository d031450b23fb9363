"""Shared by the key-frame insertion tests (not a test module): runs a case of keyframe_cases through the NumPy restatement, and compares a result - the
restatement's or the device's - with what the reference left in tests/golden/keyframe_ref.npz."""
import copy
import os

import numpy as np

import keyframe_cases as KC
import keyframe_host as KH
from planarslam_amd import keyframe as KF

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keyframe_ref.npz")
_REF = {}


def ref(name):
    if not _REF:
        with np.load(GOLDEN) as z:
            _REF.update({k: z[k] for k in z.files})
    return _REF[name]


def entries(case):
    return np.array([e[0] for e in case["entries"]], np.int32), np.array([e[1] for e in case["entries"]], np.int32)


def run_host(case, packed=None):
    """-> (the packed arrays after the call, the call's outputs), through tests/keyframe_host.py"""
    p = copy.deepcopy(KC.pack(case) if packed is None else packed)
    if case["kind"] == "need":
        out = KH.need_new_key_frame(p["map"], p["frames"], case["ref_kf"], case["params"])
    elif case["kind"] == "create":
        out = KH.create_new_key_frame(p["map"], p["graph"], p["frames"], case["create"], case["th_depth"], case["new_rank"], case["mnid"])
    else:
        out = KH.add_observations(p["map"], *entries(case), p["u_right"])
    return p, out


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), what


def check_same_state(p, q, what):
    """two packed states byte for byte: the map, the graph and the frames, padding included"""
    for part in ("map", "graph", "frames"):
        if p.get(part) is None:
            assert q.get(part) is None
            continue
        for k in p[part]:
            if k in q[part]:
                same(p[part][k], q[part][k], f"{what}: {part}.{k}")


def check_against_ref(case, before, after, out):
    """`after` / `out`: the packed state and the outputs of a call on `before`; against the reference's record of the case"""
    recs = KC.parse_ref(case, ref(case["name"]))
    m, f = after["map"], after["frames"]
    if case["kind"] == "need":
        for b, (F, r) in enumerate(zip(case["frames"], recs)):
            N, NL = len(F["match"]), len(F["lmatch"])
            for k in ("need", "interrupt_ba", "n_matches_inliers"):
                assert out[b, KF.OUT_FIELDS.index(k)] == r[k], (b, k)
            assert out[b, KF.OUT_FIELDS.index("status")] == 0
            same(f["frame_match"][b, :N], r["match"], "frame_match"); same(f["outlier"][b, :N], r["outlier"].astype(np.uint8), "outlier")
            same(f["frame_line_match"][b, :NL], r["lmatch"], "frame_line_match"); same(f["line_outlier"][b, :NL], r["loutlier"].astype(np.uint8), "line_outlier")
    elif case["kind"] == "create":
        for r in recs:
            b = r["b"]
            F = case["frames"][b]
            g, N, NL = F["map"], len(F["match"]), len(F["lmatch"])
            k, npt, nm = int(out["new_kf"][b]), int(before["map"]["n_pts"][g]), int(before["map"]["n_ml"][g])
            assert r["inserted"] == 1 and out["status"][b] == 0 and k == before["map"]["n_kf"][g]
            same(f["frame_match"][b, :N], r["match"], "frame_match"); same(m["kf_pts"][g, k, :N], r["slots"], "slots")
            same(f["frame_line_match"][b, :NL], r["lmatch"], "frame_line_match"); same(m["kf_lines"][g, k, :NL], r["lslots"], "line slots")
            for new, created, count, nobs, off, kf, n0 in ((r["new_pts"], "created_pt", "n_created_pt", "pt_nobs", "obs_off", "obs_kf", npt),
                                                          (r["new_mls"], "created_ml", "n_created_ml", "ml_nobs", "ml_obs_off", "ml_obs_kf", nm)):
                n = len(new)
                assert out[count][b] == n
                same(out[created][b, :n], new[:, 0], created)
                same(m[nobs][g, n0:n0 + n], new[:, 1], nobs)
                for c in range(n):
                    lst = m[kf][g, m[off][g, n0 + c]:m[off][g, n0 + c + 1]]
                    assert new[c, 2] == 1 and lst.tolist() == [k]
    else:
        for l, ((g, j), r) in enumerate(zip(case["entries"], recs)):
            M = KF.unpack_maps(m)[g]
            assert out["status"][l] == 0
            assert M["pt_nobs"].tolist() == r["pt_nobs"] and M["obs"] == r["obs"], "point observations"
            assert M["ml_nobs"].tolist() == r["ml_nobs"] and M["ml_obs"] == r["ml_obs"], "line observations"
            assert all(M["ml_observed"][p] == 1 for p in range(len(M["ml_nobs"])) if M["ml_nobs"][p] > 0)
            for slots, bad, added, recent in ((M["pts"][j], M["pt_bad"], out["added_pt"][l], r["recent_pts"]), (M["lines"][j], M["ml_bad"], out["added_ml"][l], r["recent_mls"])):
                assert [int(p) for i, p in enumerate(slots) if p >= 0 and not bad[p] and not added[i]] == recent, "the recent list"
                assert not added[len(slots):].any()
