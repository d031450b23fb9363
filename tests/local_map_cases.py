"""The cases of the local-map tests (not a test module): inputs of Tracking::UpdateLocalMap regenerated from seeds, each case named for what it catches.

A case is dict(maps=[M ...], frames=[F ...], local_kf_stride, short=bool).  A map M holds, unpadded: nk, kf_bad [nk], kf_rank [nk] (a permutation: the key frame's
place in pointer order), covis [nk, 10] (-1 = none), parent [nk] (-1 = none), children (nk lists, each in rank order: a std::set<KeyFrame*> iterates so), pts / lines
(nk int arrays: the slots, -1 = NULL), npts, pt_bad, obs (npts lists of key frames), nml, ml_bad, ml_observed.  A frame F holds map (index into maps), match [N],
line_match [NL] and local_in (mvpLocalKeyFrames on entry).  pack() pads a case into the arrays of planar_local_map and of planar_update_local_map; short=True asks
for output strides one below the true counts (the tests take them from the fixture).  tools/gen_golden_local_map.py feeds frame_stream() to the reference."""
import zlib

import numpy as np

NCOVIS = 10


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _children(parent, rank):
    nk = len(parent)
    ch = [[] for _ in range(nk)]
    for k in range(nk):
        if parent[k] >= 0:
            ch[parent[k]].append(k)
    return [sorted(c, key=lambda k: rank[k]) for c in ch]


def base_map(rng, nk, npts, nml, slots=(16, 64), line_slots=(4, 16), p_null=0.2, p_bad=0.1, p_bad_kf=0.0, identity_rank=False):
    """a random map whose observations are the key frames that hold the point"""
    M = dict(nk=nk, npts=npts, nml=nml)
    M["kf_bad"] = (rng.random(nk) < p_bad_kf).astype(np.uint8)
    M["kf_rank"] = np.arange(nk, dtype=np.int32) if identity_rank else rng.permutation(nk).astype(np.int32)
    cov = rng.integers(-1, nk, (nk, NCOVIS)).astype(np.int32)
    M["covis"] = cov
    M["parent"] = np.array([-1] + [int(rng.integers(0, k)) for k in range(1, nk)], np.int32)
    M["children"] = _children(M["parent"], M["kf_rank"])
    M["pts"], M["lines"] = [], []
    for k in range(nk):
        n = int(rng.integers(slots[0], slots[1] + 1))
        s = rng.integers(0, npts, n).astype(np.int32); s[rng.random(n) < p_null] = -1
        M["pts"].append(s)
        n = int(rng.integers(line_slots[0], line_slots[1] + 1))
        s = rng.integers(0, nml, n).astype(np.int32); s[rng.random(n) < p_null] = -1
        M["lines"].append(s)
    M["pt_bad"] = (rng.random(npts) < p_bad).astype(np.uint8)
    M["ml_bad"] = (rng.random(nml) < p_bad).astype(np.uint8)
    M["ml_observed"] = (rng.random(nml) < 0.8).astype(np.uint8)
    obs = [[] for _ in range(npts)]
    for k in range(nk):
        for p in np.unique(M["pts"][k]):
            if p >= 0:
                obs[p].append(k)
    M["obs"] = obs
    return M


def frame_of(rng, M, g, n=40, nl=8, from_kfs=None, local_in=()):
    """a frame whose matches are drawn from the slots of a few key frames"""
    kfs = from_kfs if from_kfs is not None else rng.choice(M["nk"], min(4, M["nk"]), replace=False)
    pool = np.concatenate([M["pts"][k] for k in kfs]); pool = pool[pool >= 0]
    lpool = np.concatenate([M["lines"][k] for k in kfs]); lpool = lpool[lpool >= 0]
    m = rng.choice(pool, n).astype(np.int32) if len(pool) else np.full(n, -1, np.int32)
    m[rng.random(n) < 0.3] = -1
    lm = rng.choice(lpool, nl).astype(np.int32) if len(lpool) else np.full(nl, -1, np.int32)
    lm[rng.random(nl) < 0.3] = -1
    return dict(map=g, match=m, line_match=lm, local_in=list(local_in))


def set_votes(M, counts):
    """points 0 .. max(counts) - 1 become good points observed so that a frame matching each of them once gives key frame k exactly counts[k] votes -> the matches"""
    top = max(counts.values())
    for i in range(top):
        M["obs"][i] = [k for k, c in sorted(counts.items()) if i < c]
        M["pt_bad"][i] = 0
    return np.arange(top, dtype=np.int32)


def by_rank(M, ranks):
    """the key frames at the given places of the pointer order"""
    inv = np.argsort(M["kf_rank"])
    return [int(inv[r]) for r in ranks]


def case_ties_and_bad_max():
    rng = _rng("ties_and_bad_max")
    M = base_map(rng, 12, 200, 40)
    assert not np.array_equal(M["kf_rank"], np.arange(12))
    a, b, c, d, e = by_rank(M, [2, 5, 7, 9, 0])
    M["kf_bad"][:] = 0
    M["kf_bad"][c] = 1                                  # the top-voted key frame is bad: neither listed nor the reference
    m = set_votes(M, {e: 3, a: 6, b: 6, c: 9, d: 4})     # a and b tie: a comes first in rank
    F = frame_of(rng, M, 0, n=0)
    F["match"] = np.concatenate([m, np.full(5, -1, np.int32)])
    return dict(maps=[M], frames=[F])


def case_empty_vote_keeps_previous():
    rng = _rng("empty_vote_keeps_previous")
    M = base_map(rng, 10, 150, 30)
    F0 = frame_of(rng, M, 0, n=20, local_in=[3, 1, 5])
    F0["match"][:] = -1
    F1 = frame_of(rng, M, 0, n=20, local_in=[7, 2, 2, 4])
    F1["match"] = rng.integers(0, 150, 20).astype(np.int32)
    M["pt_bad"][F1["match"]] = 1                        # every match is bad
    return dict(maps=[M], frames=[F0, F1])


def case_parent_ends_the_loop():
    rng = _rng("parent_ends_the_loop")
    M = base_map(rng, 14, 200, 40)
    M["kf_bad"][:] = 0
    v1, v2, v3, v4, p2, n1, n3, n4, c4 = by_rank(M, [1, 3, 6, 8, 11, 0, 2, 4, 5])
    M["covis"][:] = -1
    M["parent"][:] = -1
    M["children"] = [[] for _ in range(14)]
    M["covis"][v1, 0] = n1                              # taken
    M["parent"][v1] = v2                                # marked: the loop goes on
    M["parent"][v2] = p2                                # unmarked: appended, and the whole loop ends
    M["covis"][v3, 0] = n3                              # must not appear
    M["covis"][v4, 3] = n4
    M["children"][v4] = [c4]
    m = set_votes(M, {v1: 4, v2: 7, v3: 5, v4: 2})
    F = frame_of(rng, M, 0, n=0)
    F["match"] = m
    return dict(maps=[M], frames=[F])


def case_neighbour_child_choice():
    rng = _rng("neighbour_child_choice")
    M = base_map(rng, 16, 200, 40)
    M["kf_bad"][:] = 0
    v1, v2, v3, bad1, bad2, good1, good2, ch_bad, ch_good, ch_late, badpar, good3 = by_rank(M, [2, 4, 9, 0, 1, 3, 5, 6, 7, 8, 10, 11])
    for k in (bad1, bad2, ch_bad, badpar):
        M["kf_bad"][k] = 1
    M["covis"][:] = -1
    M["parent"][:] = -1
    ch = [[] for _ in range(16)]
    M["covis"][v1] = [bad1, v2, -1, good1, good2, -1, -1, -1, -1, -1]        # bad, marked, none, then the one taken
    ch[v1] = sorted([ch_bad, v2, ch_good, ch_late], key=lambda k: M["kf_rank"][k])   # marked, bad, taken; the later one is not
    M["covis"][v2] = [good1, bad2, -1, -1, -1, -1, -1, -1, -1, good2]        # good1 is marked by now: the last entry is taken
    M["parent"][v2] = v1                                                   # marked
    ch[v2] = [ch_good]                                                     # marked by now: none taken
    M["covis"][v3] = [-1] * 10
    ch[v3] = [ch_late]
    M["parent"][v3] = badpar                                               # a bad parent is still appended
    M["covis"][good1] = [good3] + [-1] * 9                                 # an appended key frame is not expanded
    M["children"] = ch
    m = set_votes(M, {v1: 5, v2: 3, v3: 4})
    F = frame_of(rng, M, 0, n=0)
    F["match"] = np.concatenate([np.full(3, -1, np.int32), m])
    return dict(maps=[M], frames=[F])


def case_cap_80():
    rng = _rng("cap_80")
    M = base_map(rng, 120, 600, 60, slots=(16, 24))
    M["kf_bad"][:] = 0
    order = by_rank(M, range(120))
    M["covis"][:] = -1
    M["parent"][:] = -1
    ch = [[] for _ in range(120)]
    for i in range(90):                                                    # every voted key frame has an unvoted neighbour and an unvoted child of its own
        M["covis"][order[i], 2] = order[119 - (i % 15)]
        ch[order[i]] = [order[104 - (i % 14)]]
    M["children"] = ch
    frames = []
    for nv in (79, 90):                                                    # 79: 79 -> 81 in the first iteration, stops at the second check; 90: stops at the first
        Mv = {order[i]: 1 + (i * 7) % 5 for i in range(nv)}
        F = frame_of(rng, M, 0, n=0)
        F["votes"] = Mv
        frames.append(F)
    # the two frames vote with disjoint points: 0-4 and 5-9
    for f, F in enumerate(frames):
        for i in range(5):
            M["obs"][5 * f + i] = [k for k, c in sorted(F["votes"].items()) if i < c]
            M["pt_bad"][5 * f + i] = 0
        F["match"] = np.arange(5 * f, 5 * f + 5, dtype=np.int32)
        del F["votes"]
    return dict(maps=[M], frames=frames)


def case_dedupe_across_chunks():
    rng = _rng("dedupe_across_chunks")
    M = base_map(rng, 3, 3200, 30, slots=(1500, 1500), identity_rank=False)
    M["covis"][:] = -1
    M["parent"][:] = -1
    M["children"] = [[], [], []]
    M["kf_bad"][:] = 0
    first = by_rank(M, [0])[0]
    others = [k for k in range(3) if k != first]
    M["pts"][first] = rng.permutation(3200)[:1500].astype(np.int32)
    for i, k in enumerate(others):                                         # half of a later key frame's slots repeat points of the first one, from all over it
        s = rng.integers(1600, 3200, 1500).astype(np.int32)
        rep = rng.permutation(1500)[:750]
        s[rep] = M["pts"][first][rng.permutation(1500)[:750]]
        M["pts"][k] = s
    for k in range(3):
        s = M["pts"][k]; s[rng.random(1500) < 0.15] = -1
    M["pt_bad"] = (rng.random(3200) < 0.15).astype(np.uint8)
    good = np.flatnonzero(M["pt_bad"] == 0)[:3]
    M["obs"] = [[] for _ in range(3200)]
    for p in good:
        M["obs"][p] = [0, 1, 2]
    F = frame_of(rng, M, 0, n=0)
    F["match"] = good.astype(np.int32)
    return dict(maps=[M], frames=[F])


def case_shared_map_batch():
    rng = _rng("shared_map_batch")
    maps = [base_map(rng, 20, 300, 50, p_bad_kf=0.1), base_map(rng, 27, 400, 70, p_bad_kf=0.1)]
    frames = [frame_of(rng, maps[g], g, n=int(rng.integers(30, 70)), nl=int(rng.integers(5, 15))) for g in (0, 1, 0, 0, 1)]
    return dict(maps=maps, frames=frames)


def case_overflow():
    rng = _rng("overflow")
    M = base_map(rng, 15, 250, 40)
    return dict(maps=[M], frames=[frame_of(rng, M, 0), frame_of(rng, M, 0)], short=True)


def case_lines():
    rng = _rng("lines")
    M = base_map(rng, 12, 200, 30, line_slots=(20, 40), p_bad=0.2)        # 30 lines in slots of 20-40: duplicates everywhere
    kfs = rng.choice(12, 4, replace=False)
    F = frame_of(rng, M, 0, n=40, nl=24, from_kfs=kfs)
    bad = np.flatnonzero(M["ml_bad"])[:4]
    F["line_match"][:len(bad)] = bad                                       # bad lines the frame holds: nulled
    return dict(maps=[M], frames=[F])


def case_wide_lists():
    """more key frames, key points and children than one pass of the workgroup or the wavefront covers"""
    rng = _rng("wide_lists")
    M = base_map(rng, 300, 40000, 100, slots=(16, 32), p_bad_kf=0.05)
    M["parent"][:] = -1                                                    # no parent ends the loop before the hub's turn
    hub = by_rank(M, [150])[0]
    M["kf_bad"][hub] = 0
    kids = [k for k in by_rank(M, range(40, 110)) if k != hub]             # 70 children in rank order; all but the last few are bad
    M["children"][hub] = kids
    for k in kids[:66]:
        M["kf_bad"][k] = 1
    for k in kids[66:]:
        M["kf_bad"][k] = 0
    M["covis"][hub] = -1
    F = frame_of(rng, M, 0, n=700, nl=30, from_kfs=[hub] + [int(k) for k in rng.choice(300, 6, replace=False)])
    return dict(maps=[M], frames=[F], expect_listed=[kids[66]])


CHAIN_KEYS, CHAIN_POINTS = 300, 600


def case_chain_frames():
    """two frames of CHAIN_KEYS key points on a map each of CHAIN_POINTS points: the structure under the chain test of tests/test_local_map_gpu.py, which lays
    posed frame views and projecting map points over it"""
    rng = _rng("chain_frames")
    maps = [base_map(rng, 10, CHAIN_POINTS, 20, slots=(80, 160), p_bad_kf=0.1) for _ in range(2)]
    frames = [frame_of(rng, maps[g], g, n=CHAIN_KEYS, nl=6) for g in range(2)]
    for F in frames:
        F["match"][rng.random(CHAIN_KEYS) < 0.6] = -1                     # most key points are free for the projection search
    return dict(maps=maps, frames=frames)


CASES = (("ties_and_bad_max", case_ties_and_bad_max), ("empty_vote_keeps_previous", case_empty_vote_keeps_previous),
         ("parent_ends_the_loop", case_parent_ends_the_loop), ("neighbour_child_choice", case_neighbour_child_choice), ("cap_80", case_cap_80),
         ("dedupe_across_chunks", case_dedupe_across_chunks), ("shared_map_batch", case_shared_map_batch), ("overflow", case_overflow), ("lines", case_lines),
         ("wide_lists", case_wide_lists), ("chain_frames", case_chain_frames))
NAMES = tuple(n for n, _ in CASES)


def make(name):
    c = dict(CASES)[name]()
    c.setdefault("short", False)
    c["name"] = name
    return c


def frame_stream(case, f):
    """frame f of the case as the int32 stream tools/local_map_golden/ref_local_map_main.cpp reads"""
    F = case["frames"][f]; M = case["maps"][F["map"]]
    nk = M["nk"]
    out = [[nk, M["npts"], M["nml"]], M["kf_bad"], M["kf_rank"], M["covis"].ravel(), M["parent"]]
    for lists in (M["children"], M["pts"], M["lines"]):
        out.append([len(x) for x in lists])
        out.append(np.concatenate([np.asarray(x, np.int32) for x in lists]) if nk else [])
    out += [M["pt_bad"], [len(o) for o in M["obs"]], np.concatenate([np.asarray(o, np.int32) for o in M["obs"]]), M["ml_bad"]]
    out += [[len(F["match"])], F["match"], [len(F["line_match"])], F["line_match"], [len(F["local_in"])], F["local_in"]]
    return np.concatenate([np.asarray(x, np.int32).ravel() for x in out]).astype(np.int32)


def pack(case):
    """-> (map arrays in the layout of planar_local_map for G maps, frame arrays of planar_update_local_map); the gathered rows are random, seeded by the case's name"""
    rng = _rng(case["name"] + "/rows")
    maps, frames = case["maps"], case["frames"]
    G, B = len(maps), len(frames)
    S = max(M["nk"] for M in maps) + 1
    SS = max(max(len(s) for s in M["pts"]) for M in maps) + 3
    LSS = max(max(len(s) for s in M["lines"]) for M in maps) + 1
    PS = max(M["npts"] for M in maps) + 5
    LS = max(M["nml"] for M in maps) + 2
    OC = max(sum(len(o) for o in M["obs"]) for M in maps) + 1
    CC = max(sum(len(c) for c in M["children"]) for M in maps) + 1
    m = dict(n_maps=G, kf_stride=S, slot_stride=SS, line_slot_stride=LSS, pt_stride=PS, ml_stride=LS, obs_cap=OC, child_cap=CC,
             n_kf=np.zeros(G, np.int32), kf_bad=np.zeros((G, S), np.uint8), kf_rank=np.zeros((G, S), np.int32), covis=np.full((G, S, NCOVIS), -1, np.int32),
             parent=np.full((G, S), -1, np.int32), child_off=np.zeros((G, S + 1), np.int32), child=np.full((G, CC), -7, np.int32), n_slots=np.zeros((G, S), np.int32),
             kf_pts=np.full((G, S, SS), -9, np.int32), n_line_slots=np.zeros((G, S), np.int32), kf_lines=np.full((G, S, LSS), -9, np.int32), n_pts=np.zeros(G, np.int32),
             pt_bad=np.zeros((G, PS), np.uint8), obs_off=np.zeros((G, PS + 1), np.int32), obs_kf=np.full((G, OC), -7, np.int32), n_ml=np.zeros(G, np.int32),
             ml_bad=np.zeros((G, LS), np.uint8), ml_observed=np.zeros((G, LS), np.uint8))
    m["pt_xw"] = rng.standard_normal((G, PS, 3)).astype(np.float32); m["pt_normal"] = rng.standard_normal((G, PS, 3)).astype(np.float32)
    m["pt_min_dist"] = rng.random((G, PS)).astype(np.float32); m["pt_max_dist"] = (1 + rng.random((G, PS))).astype(np.float32)
    m["pt_desc"] = rng.integers(0, 256, (G, PS, 32)).astype(np.uint8)
    m["ml_xw6"] = rng.standard_normal((G, LS, 6)); m["ml_normal"] = rng.standard_normal((G, LS, 3))
    m["ml_min_dist"] = rng.random((G, LS)).astype(np.float32); m["ml_max_dist"] = (1 + rng.random((G, LS))).astype(np.float32)
    m["ml_desc"] = rng.integers(0, 256, (G, LS, 32)).astype(np.uint8)
    for g, M in enumerate(maps):
        nk, npts, nml = M["nk"], M["npts"], M["nml"]
        m["n_kf"][g] = nk; m["n_pts"][g] = npts; m["n_ml"][g] = nml
        m["kf_bad"][g, :nk] = M["kf_bad"]; m["kf_rank"][g, :nk] = M["kf_rank"]; m["covis"][g, :nk] = M["covis"]; m["parent"][g, :nk] = M["parent"]
        off = 0
        for k in range(nk):
            c = M["children"][k]
            m["child"][g, off:off + len(c)] = c
            off += len(c)
            m["child_off"][g, k + 1] = off
            m["n_slots"][g, k] = len(M["pts"][k]); m["kf_pts"][g, k, :len(M["pts"][k])] = M["pts"][k]
            m["n_line_slots"][g, k] = len(M["lines"][k]); m["kf_lines"][g, k, :len(M["lines"][k])] = M["lines"][k]
        m["child_off"][g, nk + 1:] = off
        m["pt_bad"][g, :npts] = M["pt_bad"]; m["ml_bad"][g, :nml] = M["ml_bad"]; m["ml_observed"][g, :nml] = M["ml_observed"]
        off = 0
        for p in range(npts):
            o = M["obs"][p]
            m["obs_kf"][g, off:off + len(o)] = o
            off += len(o)
            m["obs_off"][g, p + 1] = off
        m["obs_off"][g, npts + 1:] = off
    FS = max(len(F["match"]) for F in frames) + 2
    FLS = max(len(F["line_match"]) for F in frames) + 1
    KS = case.get("local_kf_stride", S)
    f = dict(map_of=np.array([F["map"] for F in frames], np.int32), n_frame=np.array([len(F["match"]) for F in frames], np.int32),
             frame_match=np.full((B, FS), 12345, np.int32), n_frame_lines=np.array([len(F["line_match"]) for F in frames], np.int32),
             frame_line_match=np.full((B, FLS), 12345, np.int32), local_kf=np.full((B, KS), -5, np.int32), n_local_kf=np.array([len(F["local_in"]) for F in frames], np.int32))
    for b, F in enumerate(frames):
        f["frame_match"][b, :len(F["match"])] = F["match"]; f["frame_line_match"][b, :len(F["line_match"])] = F["line_match"]
        f["local_kf"][b, :len(F["local_in"])] = F["local_in"]
    return m, f
