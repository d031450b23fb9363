"""Seeded key-frame database cases shared by tools/gen_golden_kfdb.py (the REAL KeyFrameDatabase.cc + DBoW2 -> tests/golden/kfdb_ref.npz), the restatement's test and
the GPU tests.  Built only from what the repository has: synth.vocabulary / synth.vocabulary_queries for the tree and one pool of landmark descriptors, the oracle's
vocabulary transform (oracle_lib.VocabOracle) for every BowVector.  Key frames draw their features from sliding windows over the pool, so neighbours overlap, and
GetBestCovisibilityKeyFrames(10) is set from that overlap.  A case is one database: its add() / erase() calls (shuffled adds, some slots erased, one key frame added
again), then a run of queries on the same objects, first the relocalisation ones, then the loop ones."""
import numpy as np

from planarslam_amd import synth

NCOVIS = 10
# name -> parameters.  n_kf <= 70, windows of `win` features every `step`; queries are windows of the same pool at seeded offsets
CASES = {
    "db0": dict(seed=11, n_kf=70, win=(260, 420), step=45, n_reloc=8, n_loop=8, n_erase=5),
    "db1": dict(seed=12, n_kf=48, win=(200, 380), step=60, n_reloc=8, n_loop=8, n_erase=3),
    "db2": dict(seed=13, n_kf=25, win=(180, 300), step=70, n_reloc=8, n_loop=8, n_erase=2),
    "db3": dict(seed=14, n_kf=61, win=(220, 440), step=30, n_reloc=8, n_loop=8, n_erase=6),
}
VOC = dict(k=10, L=4, seed=81)
KF_STRIDE, WORD_STRIDE = 80, 448
FIRST_QUERY_ID = 1000          # Frame / KeyFrame mnId of the queries: unique, and never 0 (the constructors' mnRelocQuery(0) / mnLoopQuery(0))

_VOC = None
_BUILT = {}


def vocabulary():
    global _VOC
    if _VOC is None:
        _VOC = synth.vocabulary(**VOC)
    return _VOC


def _bow(oracle, desc):
    t = oracle.transform(desc)
    return t["bow_word"].astype(np.int32), t["bow_value"].astype(np.float64)


def build(name):
    """-> dict(n_kf, kf_bow [(word, value)], covis [n_kf, 10], ops [(0 add | 1 erase, slot)], queries [dict(mode, id, word, value, excluded [n_kf] u8, min_score f32,
    desc [n, 32] the features behind word / value)])"""
    if name in _BUILT:
        return _BUILT[name]
    import oracle_lib as ol
    p = CASES[name]
    rng = np.random.default_rng(p["seed"])
    voc = vocabulary()
    oracle = ol.VocabOracle(voc)
    n_kf, step = p["n_kf"], p["step"]
    starts = np.arange(n_kf) * step + rng.integers(0, step // 2, n_kf)
    sizes = rng.integers(p["win"][0], p["win"][1], n_kf)
    pool = synth.vocabulary_queries(voc, int((starts + sizes).max()) + 1, p["seed"] + 100)
    kf_bow = [_bow(oracle, pool[s:s + z]) for s, z in zip(starts, sizes)]
    assert all(len(w) <= WORD_STRIDE for w, _ in kf_bow)
    overlap = np.zeros((n_kf, n_kf), np.int64)
    for i in range(n_kf):
        for j in range(n_kf):
            if i != j:
                overlap[i, j] = max(0, min(starts[i] + sizes[i], starts[j] + sizes[j]) - max(starts[i], starts[j]))
    covis = np.full((n_kf, NCOVIS), -1, np.int32)
    for i in range(n_kf):
        order = sorted((j for j in range(n_kf) if overlap[i, j] > 0), key=lambda j: (-overlap[i, j], j))[:NCOVIS]
        covis[i, :len(order)] = order
    ops = [(0, int(j)) for j in rng.permutation(n_kf)]
    erased = [int(j) for j in rng.choice(n_kf, p["n_erase"], replace=False)]
    ops += [(1, j) for j in erased] + [(0, erased[0])]
    queries = []
    for q in range(p["n_reloc"] + p["n_loop"]):
        mode = 0 if q < p["n_reloc"] else 1
        s = int(rng.integers(0, starts[-1]))
        z = int(rng.integers(p["win"][0] // 2, p["win"][1]))
        desc = pool[s:s + z]
        if q % 3 == 2:                                          # a sparser view of the same place
            desc = desc[rng.random(len(desc)) < 0.6]
        w, v = _bow(oracle, desc)
        excluded = np.zeros(n_kf, np.uint8)
        min_score = np.float32(0)
        if mode == 1:
            ov = np.array([max(0, min(s + z, starts[j] + sizes[j]) - max(s, starts[j])) for j in range(n_kf)])
            excluded[ov > 0.7 * z] = 1                          # the query key frame's connected key frames
            # the minimum score over the connected key frames: now low, now above some of the scored ones (and sometimes above all of them)
            min_score = np.float32(rng.uniform(0.01, 0.12) if q % 2 == 0 else rng.uniform(0.3, 0.75))
        queries.append(dict(mode=mode, id=FIRST_QUERY_ID + q, word=w, value=v, excluded=excluded, min_score=min_score, desc=desc))
    case = dict(n_kf=n_kf, kf_bow=kf_bow, covis=covis, ops=ops, queries=queries)
    _BUILT[name] = case
    return case


def score_pairs(case):
    """(a, b) pairs of BowVectors for Vocabulary::score: index < n_kf is a key frame, n_kf + q a query"""
    n, nq = case["n_kf"], len(case["queries"])
    pairs = [(n + q, (7 * q) % n) for q in range(nq)] + [(j, (j + 1) % n) for j in range(0, n, 5)] + [(0, n - 1), (n + 0, n + 0)]
    return np.array(pairs, np.int32)


def bow_of(case, i):
    return case["kf_bow"][i] if i < case["n_kf"] else (case["queries"][i - case["n_kf"]]["word"], case["queries"][i - case["n_kf"]]["value"])


def database_arrays(case, kf_stride=KF_STRIDE, word_stride=WORD_STRIDE):
    """the padded arrays of one database after the case's add() / erase() calls (slot = key frame index)"""
    n = case["n_kf"]
    d = dict(n_kf=np.int32(n), present=np.zeros(kf_stride, np.uint8), add_seq=np.zeros(kf_stride, np.int32), bow_n=np.zeros(kf_stride, np.int32),
             bow_word=np.zeros((kf_stride, word_stride), np.int32), bow_value=np.zeros((kf_stride, word_stride)), covis=np.full((kf_stride, NCOVIS), -1, np.int32))
    for j, (w, v) in enumerate(case["kf_bow"]):
        d["bow_n"][j] = len(w); d["bow_word"][j, :len(w)] = w; d["bow_value"][j, :len(w)] = v
    d["covis"][:n] = case["covis"]
    for seq, (op, j) in enumerate(case["ops"]):
        d["present"][j] = 1 if op == 0 else 0
        if op == 0:
            d["add_seq"][j] = seq
    return d


def stacked_databases(names=None):
    """the databases of the cases as one view of G = len(names) databases -> dict of [G, ...] arrays"""
    ds = [database_arrays(build(n)) for n in (names or list(CASES))]
    return {k: np.stack([d[k] for d in ds]) for k in ds[0]}


def query_arrays(queries, stride=WORD_STRIDE):
    B = len(queries)
    n = np.array([len(q["word"]) for q in queries], np.int32)
    w = np.zeros((B, stride), np.int32); v = np.zeros((B, stride))
    for b, q in enumerate(queries):
        w[b, :n[b]] = q["word"]; v[b, :n[b]] = q["value"]
    return n, w, v


def write_input(path, case, pairs):
    """the input of the fixture generator's driver (tools/kfdb_golden/ref_kfdb_main.cpp, which documents the format) and of tests/adapter_shim/adapter_kfdb_main.cpp"""
    n = case["n_kf"]
    with open(path, "wb") as f:
        i32 = lambda *a: f.write(np.array(a, "<i4").tobytes())
        i32(n, len(case["ops"]), len(case["queries"]), len(pairs))
        for (w, v), c in zip(case["kf_bow"], case["covis"]):
            i32(len(w)); f.write(w.astype("<i4").tobytes()); f.write(v.astype("<f8").tobytes()); f.write(c.astype("<i4").tobytes())
        for op, j in case["ops"]:
            i32(op, j)
        for q in case["queries"]:
            i32(q["mode"], q["id"], len(q["word"])); f.write(q["word"].astype("<i4").tobytes()); f.write(q["value"].astype("<f8").tobytes())
            f.write(np.float32(q["min_score"]).tobytes()); f.write(q["excluded"].astype(np.uint8).tobytes())
        f.write(np.asarray(pairs, "<i4").tobytes())


def read_output(path, case, n_pairs):
    """what either driver wrote -> dict(score_in, score, common [nq, KF_STRIDE], cand, n_cand, n_scored, pair_score)"""
    n, nq, S = case["n_kf"], len(case["queries"]), KF_STRIDE
    buf = open(path, "rb").read()
    out = dict(score_in=np.zeros((nq, S), np.float32), score=np.zeros((nq, S), np.float32), common=np.zeros((nq, S), np.int32), cand=np.full((nq, S), -1, np.int32),
               n_cand=np.zeros(nq, np.int32), n_scored=np.zeros(nq, np.int32))
    off = 0
    def take(dt, k):
        nonlocal off
        a = np.frombuffer(buf, dt, k, off); off += a.nbytes
        return a
    for q in range(nq):
        out["score_in"][q, :n] = take("<f4", n)
        k = int(take("<i4", 1)[0]); out["n_cand"][q] = k; out["cand"][q, :k] = take("<i4", k)
        out["common"][q, :n] = take("<i4", n); out["score"][q, :n] = take("<f4", n); out["n_scored"][q] = take("<i4", 1)[0]
    out["pair_score"] = take("<f8", n_pairs).copy()
    assert off == len(buf)
    return out
