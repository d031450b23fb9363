"""The cases of the covisibility-graph tests (not a test module): inputs of KeyFrame::UpdateConnections regenerated from seeds, each case named for what it catches.

A case is dict(maps=[M ...], entries=[(map, key frame) ...]).  A map M holds, unpadded: nk, kf_rank [nk] (a permutation: the key frame's place in pointer order),
pts (nk int arrays: the slots, -1 = NULL), npts, pt_bad, obs (npts lists of key frames), and the connection state on entry: conn_w [nk, nk] (0 = absent), ord_kf /
ord_w (nk lists), first [nk] (mbFirstConnection), mnid [nk], parent [nk] (-1 = none).  pack() pads a case into the arrays of planar_local_map the call reads and of
planar_covis_graph; tools/gen_golden_connections.py feeds stream() to the reference."""
import zlib

import numpy as np

from planarslam_amd import connections as CN

TH = 15


def _rng(name):
    return np.random.default_rng(zlib.crc32(("connections/" + name).encode()))


def blank_map(nk, rank=None):
    """nk key frames without slots, points or connections; key frame k has mnId k and has never been connected"""
    return dict(nk=nk, kf_rank=np.arange(nk, dtype=np.int32) if rank is None else np.asarray(rank, np.int32), pts=[np.zeros(0, np.int32) for _ in range(nk)], npts=0,
                pt_bad=np.zeros(0, np.uint8), obs=[], conn_w=np.zeros((nk, nk), np.int32), ord_kf=[[] for _ in range(nk)], ord_w=[[] for _ in range(nk)],
                first=np.ones(nk, np.uint8), mnid=np.arange(nk, dtype=np.int32), parent=np.full(nk, -1, np.int32))


def scrambled(rng, nk):
    while True:
        r = rng.permutation(nk).astype(np.int32)
        if not np.array_equal(r, np.arange(nk)):
            return r


def add_point(M, observers, holders=None, bad=False):
    """a new map point observed by `observers` and held in one new slot of each of `holders` (default: the observers) -> its id"""
    p = M["npts"]
    M["npts"] += 1
    M["pt_bad"] = np.append(M["pt_bad"], np.uint8(bad))
    M["obs"].append([int(k) for k in observers])
    for k in (observers if holders is None else holders):
        M["pts"][k] = np.append(M["pts"][k], np.int32(p))
    return p


def share(M, a, b, n):
    """n new good points seen by key frames a and b"""
    return [add_point(M, (a, b)) for _ in range(n)]


def null_slots(M, k, n=1):
    M["pts"][k] = np.append(M["pts"][k], np.full(n, -1, np.int32))


def connect(M, x, weights):
    """key frame x comes in with the row `weights` ({key frame: weight}) and its full ordered list"""
    M["conn_w"][x] = 0
    for k, w in weights.items():
        M["conn_w"][x, k] = w
    order = sorted(weights, key=lambda k: (weights[k], M["kf_rank"][k]), reverse=True)
    M["ord_kf"][x] = [int(k) for k in order]; M["ord_w"][x] = [int(weights[k]) for k in order]
    M["first"][x] = 0


def shuffle_slots(rng, M):
    for k in range(M["nk"]):
        M["pts"][k] = rng.permutation(M["pts"][k]).astype(np.int32)


def case_pair():
    M = blank_map(2)
    share(M, 0, 1, 20)
    return dict(maps=[M], entries=[(0, 1)])


def case_threshold():
    rng = _rng("threshold")
    M = blank_map(4, scrambled(rng, 4))
    for k, n in ((1, TH - 1), (2, TH), (3, TH + 1)):
        share(M, 0, k, n)
    shuffle_slots(rng, M)
    return dict(maps=[M], entries=[(0, 0)], j=0, counts={1: TH - 1, 2: TH, 3: TH + 1})


def case_fallback_max():
    rng = _rng("fallback_max")
    M = blank_map(6, scrambled(rng, 6))
    counts = {1: 5, 2: 9, 3: 3, 4: 9, 5: 1}
    for k, n in counts.items():
        share(M, 0, k, n)
    shuffle_slots(rng, M)
    return dict(maps=[M], entries=[(0, 0)], j=0, counts=counts)


def case_ties():
    rng = _rng("ties")
    M = blank_map(7, scrambled(rng, 7))
    counts = {1: 17, 2: 20, 3: 17, 4: 17, 5: 20, 6: 16}
    for k, n in counts.items():
        share(M, 0, k, n)
    shuffle_slots(rng, M)
    return dict(maps=[M], entries=[(0, 0)], j=0, counts=counts)


def case_asymmetric():
    rng = _rng("asymmetric")
    M = blank_map(5, scrambled(rng, 5))
    j, a, b, c, d = 0, 1, 2, 3, 4
    pa = share(M, j, a, TH - 1)
    M["pts"][j] = np.append(M["pts"][j], np.int32(pa[0]))          # one point in two slots: a reaches the threshold by the repeat
    for _ in range(TH):
        add_point(M, (b,), holders=(j, b))                        # j holds the points but their lists lack j: they count all the same
    share(M, j, c, TH - 1)
    for _ in range(6):
        add_point(M, (j, c), bad=True)                            # bad points do not count: c stays one below the threshold
    share(M, j, d, TH + 2)                                         # every one of these lists j itself: a self observation is skipped
    null_slots(M, j, 7)
    shuffle_slots(rng, M)
    return dict(maps=[M], entries=[(0, j)], j=j, counts={a: TH, b: TH, c: TH - 1, d: TH + 2})


def case_sequence():
    rng = _rng("sequence")
    M = blank_map(9, scrambled(rng, 9))
    A, B, C, D, E, F, U, Z, Y = range(9)
    ab = share(M, A, B, 20)
    M["pts"][B] = np.append(M["pts"][B], np.int32(ab[3]))          # B counts A 21 times, A counts B 20 times: B's AddConnection on A changes A's row
    share(M, A, C, 5)                                              # A's sub-threshold neighbour: in A's list only after B re-sorted it in full
    share(M, D, E, 18)                                             # the same weight from both sides: E's AddConnection leaves D alone
    share(M, D, F, 4)                                              # so D's sub-threshold neighbour never shows
    share(M, A, U, 16)
    connect(M, U, {A: 3, Z: 9, Y: 9})                              # not listed; its stale weight for A is overridden and the whole row listed
    connect(M, Z, {U: 9}); connect(M, Y, {U: 9})
    connect(M, B, {F: 40})                                         # listed: the stale row vanishes
    M["parent"][B] = F
    shuffle_slots(rng, M)
    return dict(maps=[M], entries=[(0, A), (0, D), (0, B), (0, C), (0, E)], names=dict(A=A, B=B, C=C, D=D, E=E, F=F, U=U, Z=Z, Y=Y))


def case_parents():
    rng = _rng("parents")
    rank = scrambled(rng, 6)
    zero = int(np.flatnonzero(rank == 3)[0])                       # the key frame with mnId 0 sits in the middle of the pointer order
    M = blank_map(6, rank)
    M["mnid"] = np.array([k + 1 for k in range(6)], np.int32); M["mnid"][zero] = 0
    others = [k for k in range(6) if k != zero]
    old, new, p_old, p_new = others[:4]
    share(M, zero, new, 25); share(M, zero, old, 16)
    share(M, new, p_new, 30)                                       # the front of new's list: its parent
    share(M, old, p_new, 30)
    connect(M, old, {p_old: 2})                                    # connected before: keeps p_old although p_new leads its list now
    M["parent"][old] = p_old
    shuffle_slots(rng, M)
    return dict(maps=[M], entries=[(0, zero), (0, old), (0, new)], names=dict(zero=zero, old=old, new=new, p_old=p_old, p_new=p_new))


def case_empty():
    rng = _rng("empty")
    M = blank_map(4, scrambled(rng, 4))
    share(M, 1, 2, 16)
    for _ in range(5):
        add_point(M, (0, 3), bad=True)
    for _ in range(3):
        add_point(M, (0,))                                         # seen by nobody else
    null_slots(M, 0, 4)
    connect(M, 0, {3: 6, 2: 1})
    M["parent"][0] = 3
    M["first"][0] = 1                                              # would take a parent if the call went on
    return dict(maps=[M], entries=[(0, 0), (0, 1)])


def random_map(rng, nk, npts, per_point=3, p_bad=0.1, p_null=0.1):
    M = blank_map(nk, scrambled(rng, nk))
    for _ in range(npts):
        add_point(M, rng.choice(nk, per_point, replace=False), bad=rng.random() < p_bad)
    for k in range(nk):
        null_slots(M, k, int(rng.integers(0, 1 + int(p_null * len(M["pts"][k])))))
    shuffle_slots(rng, M)
    return M


def case_two_maps():
    rng = _rng("two_maps")
    maps = [random_map(rng, 8, 300), random_map(rng, 11, 420)]
    connect(maps[0], 2, {0: 4, 5: 50}); connect(maps[1], 7, {1: 15, 2: 15, 9: 3})
    return dict(maps=maps, entries=[(0, 3), (1, 10), (0, 0), (1, 2), (1, 7), (0, 6), (1, 0)])


WIDE_KEYFRAMES, WIDE_SLOTS, WIDE_OBS = 1024, 2000, 40


def case_wide():
    """more key frames than one pass of a workgroup, one bitonic tile or one LDS row of 64 bins covers: key frame `hub` is connected to all the others"""
    rng = _rng("wide")
    nk = WIDE_KEYFRAMES
    M = blank_map(nk, scrambled(rng, nk))
    hub = 517
    others = np.array([k for k in range(nk) if k != hub])
    w = np.linspace(0.1, 1.0, nk - 1); w /= w.sum()
    obs = [others[rng.choice(nk - 1, WIDE_OBS, replace=False, p=w)] for _ in range(WIDE_SLOTS)]
    M["npts"] = WIDE_SLOTS; M["pt_bad"] = np.zeros(WIDE_SLOTS, np.uint8); M["obs"] = [[int(k) for k in o] for o in obs]
    M["pts"][hub] = rng.permutation(WIDE_SLOTS).astype(np.int32)
    counts = np.bincount(np.concatenate(obs), minlength=nk)
    assert (np.delete(counts, hub) > 0).all() and (counts[others] < TH).any() and (counts >= TH).sum() > 512
    connect(M, int(others[0]), {int(others[5]): 1000})
    return dict(maps=[M], entries=[(0, hub)], hub=hub, counts=counts)


CASES = (("pair", case_pair), ("threshold", case_threshold), ("fallback_max", case_fallback_max), ("ties", case_ties), ("asymmetric", case_asymmetric),
         ("sequence", case_sequence), ("parents", case_parents), ("empty", case_empty), ("two_maps", case_two_maps), ("wide", case_wide))
NAMES = tuple(n for n, _ in CASES)
_made = {}


def make(name):
    """the case, built once; nobody changes it"""
    if name not in _made:
        c = dict(CASES)[name]()
        c["name"] = name
        _made[name] = c
    return _made[name]


def state_of(M):
    return dict(conn_w=M["conn_w"], ord_kf=M["ord_kf"], ord_w=M["ord_w"], first=M["first"], mnid=M["mnid"], parent=M["parent"])


def stream(case):
    """the case as the int32 stream tools/connections_golden/ref_connections_main.cpp reads"""
    out = [[len(case["maps"])]]
    cat = lambda lists: np.concatenate([np.asarray(x, np.int32).ravel() for x in lists] + [np.zeros(0, np.int32)])
    for M in case["maps"]:
        nk = M["nk"]
        out += [[nk, M["npts"]], M["kf_rank"], M["mnid"], M["first"], M["parent"], [len(s) for s in M["pts"]], cat(M["pts"]), M["pt_bad"], [len(o) for o in M["obs"]],
                cat(M["obs"])]
        rows = [[(k, M["conn_w"][x, k]) for k in np.flatnonzero(M["conn_w"][x])] for x in range(nk)]
        out += [[len(r) for r in rows], cat(rows), [len(o) for o in M["ord_kf"]], cat([np.stack([M["ord_kf"][x], M["ord_w"][x]], 1) for x in range(nk)])]
    out += [[len(case["entries"])], np.asarray(case["entries"], np.int32)]
    return cat(out)


def pack(case):
    """-> (the arrays of planar_local_map the call reads, for G maps; the arrays of planar_covis_graph; entry_map, entry_kf).  Padding holds out-of-range values."""
    maps = case["maps"]
    G = len(maps)
    S = min(max(M["nk"] for M in maps) + 1, 1024)
    SS = max(max(len(s) for s in M["pts"]) for M in maps) + 3
    PS = max(M["npts"] for M in maps) + 5
    OC = max(sum(len(o) for o in M["obs"]) for M in maps) + 1
    m = dict(n_kf=np.zeros(G, np.int32), kf_rank=np.full((G, S), -4, np.int32), n_slots=np.zeros((G, S), np.int32), kf_pts=np.full((G, S, SS), -9, np.int32),
             n_pts=np.zeros(G, np.int32), pt_bad=np.zeros((G, PS), np.uint8), obs_off=np.zeros((G, PS + 1), np.int32), obs_kf=np.full((G, OC), -7, np.int32))
    for g, M in enumerate(maps):
        nk, npts = M["nk"], M["npts"]
        m["n_kf"][g] = nk; m["n_pts"][g] = npts; m["kf_rank"][g, :nk] = M["kf_rank"]; m["pt_bad"][g, :npts] = M["pt_bad"]
        for k in range(nk):
            m["n_slots"][g, k] = len(M["pts"][k]); m["kf_pts"][g, k, :len(M["pts"][k])] = M["pts"][k]
        off = 0
        for p in range(npts):
            o = M["obs"][p]
            m["obs_kf"][g, off:off + len(o)] = o
            off += len(o)
            m["obs_off"][g, p + 1] = off
        m["obs_off"][g, npts + 1:] = off
    e = np.asarray(case["entries"], np.int32)
    return m, CN.pack_graph([state_of(M) for M in maps], S), e[:, 0].copy(), e[:, 1].copy()
