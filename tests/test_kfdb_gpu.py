"""GPU parity (bit-exact, no tolerance): planar_kfdb_detect and planar_bow_score, both flavours, against the fixture from the real reference
(tests/golden/kfdb_ref.npz: src/KeyFrameDatabase.cc + the vendored DBoW2) and against tests/host_shim/kfdb_host.cpp."""
import ctypes as C

import numpy as np
import pytest

import kfdb_cases as KC
import kfdb_host as KH

pytestmark = pytest.mark.gpu
NAMES = list(KC.CASES)
S, W = KC.KF_STRIDE, KC.WORD_STRIDE
CAND_SENTINEL, SCORE_SENTINEL = 777, np.float32(7.5)


@pytest.fixture(scope="module")
def host():
    return KH.load_host()


@pytest.fixture(scope="module")
def ctx():
    from planarslam_amd._lib import Context
    return Context(0)


@pytest.fixture(scope="module")
def batch():
    """4 databases (25 .. 70 key frames in a kf_stride of 80, 180 .. 420 words in a word_stride of 448 = 7 x 64) and, per mode, 32 queries that share them, with the score members
    the real reference held before each query; slots beyond n_kf hold a sentinel score"""
    G = KH.golden()
    db = KC.stacked_databases(NAMES)
    modes = {}
    for mode in (0, 1):
        qs, q_db, score_in, ref = [], [], [], dict(score=[], common=[], n_cand=[], cand=[], n_scored=[])
        for g, name in enumerate(NAMES):
            case = KC.build(name)
            for i, q in enumerate(case["queries"]):
                if q["mode"] != mode:
                    continue
                qs.append(q); q_db.append(g)
                pad = np.arange(S) >= case["n_kf"]
                score_in.append(np.where(pad, SCORE_SENTINEL, G[name + "_score_in"][i]))
                ref["score"].append(np.where(pad, SCORE_SENTINEL, G[name + "_score"][i]))
                for k in ("common", "n_cand", "cand", "n_scored"):
                    ref[k].append(G[f"{name}_{k}"][i])
        n, w, v = KC.query_arrays(qs)
        ex = np.zeros((len(qs), S), np.uint8)
        for b, q in enumerate(qs):
            ex[b, :len(q["excluded"])] = q["excluded"]
        modes[mode] = dict(queries=qs, q_db=np.array(q_db, np.int32), n=n, word=w, value=v, excluded=ex, min_score=np.array([q["min_score"] for q in qs], np.float32),
                           score_in=np.stack(score_in).astype(np.float32), ref={k: np.stack(a) for k, a in ref.items()})
    return db, modes


class Device:
    """torch device copies, for the _dev flavours"""

    def __init__(self):
        import torch
        self.torch, self.dev, self.keep = torch, torch.device("cuda", 0), []

    def up(self, a):
        if a is None:
            return None
        self.keep.append(self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(self.dev))
        return self.keep[-1].data_ptr()

    def database(self, db):
        from planarslam_amd import kfdb
        v, arrays = kfdb.kf_database(db)
        for name, a in arrays.items():
            setattr(v, name, self.up(a))
        return v

    def down(self, i, like):
        return self.keep[i].cpu().numpy().view(like.dtype).reshape(like.shape)


def run_dev(ctx, mode, db, q_db, n, w, v, ex, ms, score, cand):
    from planarslam_amd._lib import check, lib
    d = Device()
    view = d.database(db)
    B = len(q_db)
    ins = [d.up(a) for a in (q_db, n, w, v)]
    d_ex, d_ms = d.up(ex), d.up(ms)
    first = len(d.keep)
    outs = [d.up(score), d.up(np.full((B, view.kf_stride), -5, np.int32)), d.up(np.full(B, -5, np.int32)), d.up(cand), d.up(np.full(B, -5, np.int32))]
    d.torch.cuda.synchronize()
    check(lib().planar_kfdb_detect_dev(ctx.h, mode, C.byref(view), B, *ins, w.shape[-1], d_ex, d_ms, *outs))
    ctx.sync()
    return dict(score=d.down(first, score), common_words=d.down(first + 1, np.zeros((B, view.kf_stride), np.int32)), n_cand=d.down(first + 2, np.zeros(B, np.int32)),
                cand=d.down(first + 3, cand), n_scored=d.down(first + 4, np.zeros(B, np.int32)))


def run(ctx, flavour, mode, db, q_db, n, w, v, ex, ms, score, cand):
    from planarslam_amd import kfdb
    if flavour == "host":
        return kfdb.detect(ctx, mode, db, q_db, n, w, v, ex, ms, score=score, cand=cand)
    return run_dev(ctx, mode, db, q_db, n, w, v, ex, ms, score, cand)


def host_rows(host, mode, db, q_db, n, w, v, ex, ms, score):
    """the restatement, query by query, each on its own score row"""
    rows = []
    for b in range(len(q_db)):
        one = {k: a[q_db[b]] for k, a in db.items()}
        rows.append(KH.host_detect(host, one, mode, w[b, :n[b]], v[b, :n[b]], None if ex is None else ex[b], 0 if ms is None else ms[b], score[b], report=False))
    return rows


def assert_equals_host(got, rows, cand_init):
    for b, r in enumerate(rows):
        k = r["n_cand"]
        assert got["n_cand"][b] == k and got["n_scored"][b] == r["n_scored"], b
        assert got["cand"][b, :k].tolist() == r["cand"][:k].tolist(), b
        assert (got["cand"][b, k:] == cand_init[b, k:]).all(), b
        assert got["common_words"][b].tolist() == r["common"].tolist(), b
        assert got["score"][b].view(np.uint32).tolist() == r["score"].view(np.uint32).tolist(), b


def widen(a, stride):
    """the last axis of a padded array zero-filled up to `stride`"""
    return np.concatenate([a, np.zeros(a.shape[:-1] + (stride - a.shape[-1],), a.dtype)], -1)


@pytest.mark.parametrize("flavour", ["host", "dev"])
@pytest.mark.parametrize("word_stride", [448, 450])
@pytest.mark.parametrize("mode", [0, 1])
def test_detect_equals_the_reference_and_the_restatement(ctx, host, batch, mode, word_stride, flavour):
    """word_stride 448 is seven full chunks of 64 lanes (the vectors themselves, 66 .. 420 words, end inside a chunk); 450 is the same data in a stride that is no
    multiple of 64, nor of 4: rows of bow_word then start off a 16-byte boundary"""
    db, modes = batch
    m = modes[mode]
    B = len(m["q_db"])
    assert B == 32 and db["bow_word"].shape == (4, 80, 448) and (db["bow_n"] % 64 != 0).any() and (m["n"] % 64 != 0).any()
    if word_stride != 448:
        assert word_stride % 64 != 0
        db = dict(db, bow_word=widen(db["bow_word"], word_stride), bow_value=widen(db["bow_value"], word_stride))
        m = dict(m, word=widen(m["word"], word_stride), value=widen(m["value"], word_stride))
    cand0 = np.full((B, S), CAND_SENTINEL, np.int32)
    ex, ms = (m["excluded"], m["min_score"]) if mode else (None, None)
    got = run(ctx, flavour, mode, db, m["q_db"], m["n"], m["word"], m["value"], ex, ms, m["score_in"], cand0)
    ref = m["ref"]
    np.testing.assert_array_equal(got["n_cand"], ref["n_cand"])
    np.testing.assert_array_equal(got["n_scored"], ref["n_scored"])
    np.testing.assert_array_equal(got["common_words"], ref["common"])
    np.testing.assert_array_equal(got["score"].view(np.uint32), ref["score"].view(np.uint32))       # assigned where the reference assigns, untouched elsewhere (sentinels too)
    for b in range(B):
        k = ref["n_cand"][b]
        assert got["cand"][b, :k].tolist() == ref["cand"][b, :k].tolist(), b
        assert (got["cand"][b, k:] == CAND_SENTINEL).all(), b
    assert_equals_host(got, host_rows(host, mode, db, m["q_db"], m["n"], m["word"], m["value"], ex, ms, m["score_in"]), cand0)
    assert ref["n_cand"].max() >= 2 and (got["score"] == SCORE_SENTINEL).any()


@pytest.mark.parametrize("flavour", ["host", "dev"])
def test_degenerate_queries_give_no_candidate_and_leave_the_scores(ctx, host, flavour):
    db = KC.stacked_databases(["db2"])
    db = {k: np.concatenate([a, np.zeros_like(a)]) for k, a in db.items()}           # database 1: n_kf == 0
    case = KC.build("db2")
    q = case["queries"][0]
    used = np.unique(np.concatenate([w for w, _ in case["kf_bow"]]))
    foreign = np.setdiff1d(np.arange(used.max() + 200, dtype=np.int32), used)[:150]    # words no key frame holds
    n, w, v = KC.query_arrays([q, q, dict(word=foreign, value=np.full(150, 1 / 150)), q])
    n[1] = 0                                                                         # a query without words
    q_db = np.array([1, 0, 0, 0], np.int32)
    score0 = np.full((4, S), SCORE_SENTINEL, np.float32)
    cand0 = np.full((4, S), CAND_SENTINEL, np.int32)
    for mode, rows in ((0, (0, 1, 2)), (1, (0, 1, 2, 3))):
        ex = np.zeros((4, S), np.uint8); ex[3] = 1                                   # loop mode: every sharer is connected to the query
        ms = np.full(4, 0.05, np.float32)
        got = run(ctx, flavour, mode, db, q_db, n, w, v, ex if mode else None, ms if mode else None, score0, cand0)
        for b in rows:
            assert got["n_cand"][b] == 0 and got["n_scored"][b] == 0, (mode, b)
            assert (got["score"][b] == SCORE_SENTINEL).all() and (got["cand"][b] == CAND_SENTINEL).all() and (got["common_words"][b] == 0).all(), (mode, b)
        assert_equals_host(got, host_rows(host, mode, db, q_db, n, w, v, ex if mode else None, ms if mode else None, score0), cand0)
        if mode == 0:
            assert got["n_cand"][3] >= 1                                             # the same query, not excluded, finds its place


def big_vectors(seed, top=10 ** 6):
    """two 4096-word BowVectors over the word range of a k = 10, L = 6 tree, both reaching its last word"""
    rng = np.random.default_rng(seed)
    a = np.sort(rng.choice(top - 1, 4095, replace=False)).astype(np.int32)
    keep = rng.random(4095) < 0.9
    extra = np.setdiff1d(rng.choice(top - 1, 3000, replace=False), a)[:4095 - int(keep.sum())]
    b = np.sort(np.concatenate([a[keep], extra])).astype(np.int32)
    a, b = np.append(a, top - 1).astype(np.int32), np.append(b, top - 1).astype(np.int32)
    va, vb = rng.uniform(0.5, 9.0, 4096), rng.uniform(0.5, 9.0, 4096)
    return (a, va / va.sum()), (b, vb / vb.sum())


@pytest.mark.parametrize("flavour", ["host", "dev"])
def test_one_key_frame_and_one_query_at_the_word_limit(ctx, host, flavour):
    kf, q = big_vectors(5)
    assert len(kf[0]) == len(q[0]) == 4096 and kf[0][-1] == q[0][-1] == 999999 and len(np.intersect1d(kf[0], q[0])) > 2000
    db = dict(n_kf=np.ones(1, np.int32), present=np.ones((1, 1), np.uint8), add_seq=np.zeros((1, 1), np.int32), bow_n=np.full((1, 1), 4096, np.int32),
              bow_word=kf[0].reshape(1, 1, 4096), bow_value=kf[1].reshape(1, 1, 4096), covis=np.full((1, 1, 10), -1, np.int32))
    n, w, v = np.array([4096], np.int32), q[0][None], q[1][None]
    score0, cand0 = np.full((1, 1), SCORE_SENTINEL, np.float32), np.full((1, 1), CAND_SENTINEL, np.int32)
    q_db = np.zeros(1, np.int32)
    for mode in (0, 1):
        ex, ms = (np.zeros((1, 1), np.uint8), np.array([0.01], np.float32)) if mode else (None, None)
        got = run(ctx, flavour, mode, db, q_db, n, w, v, ex, ms, score0, cand0)
        assert got["n_cand"][0] == 1 and got["cand"][0, 0] == 0 and got["n_scored"][0] == 1 and got["common_words"][0, 0] == len(np.intersect1d(kf[0], q[0]))
        assert_equals_host(got, host_rows(host, mode, db, q_db, n, w, v, ex, ms, score0), cand0)


@pytest.mark.parametrize("flavour", ["host", "dev"])
def test_bow_score_equals_the_reference_and_the_restatement(ctx, host, flavour):
    from planarslam_amd import kfdb
    from planarslam_amd._lib import check, lib
    G = KH.golden()
    bows, want = [], []
    for name in NAMES:
        case = KC.build(name)
        bows += [KC.bow_of(case, a) + KC.bow_of(case, b) for a, b in KC.score_pairs(case)]
        want.append(G[name + "_pair_score"])
    kf, q = big_vectors(6)
    low, high = (np.arange(0, 300, 2, dtype=np.int32), np.full(150, 1 / 150)), (np.arange(1, 301, 2, dtype=np.int32), np.full(150, 1 / 150))
    empty = (np.zeros(0, np.int32), np.zeros(0))
    bows += [q + kf, kf + q, low + high, empty + low, low + empty]                   # the word limit; no common word (-0.0); an empty vector on either side
    ref, (an, aw, av, sa, bn, bw, bv, sb) = KH.host_bow_score(host, bows)
    assert sa == sb == 4096 and np.signbit(ref[-3]) and ref[-3] == 0
    if flavour == "host":
        got = kfdb.bow_score(ctx, an, aw, av, bn, bw, bv)
    else:
        d = Device()
        ptrs = [d.up(a) for a in (an, aw, av)] + [sa] + [d.up(a) for a in (bn, bw, bv)] + [sb, d.up(np.zeros(len(an)))]
        d.torch.cuda.synchronize()
        check(lib().planar_bow_score_dev(ctx.h, len(an), *ptrs))
        ctx.sync()
        got = d.down(len(d.keep) - 1, np.zeros(len(an)))
    np.testing.assert_array_equal(got.view(np.uint64), ref.view(np.uint64))
    np.testing.assert_array_equal(got[:-5].view(np.uint64), np.concatenate(want).view(np.uint64))


def test_vocabulary_score_is_the_references_double(ctx):
    from planarslam_amd.bow import ORBVocabulary
    G = KH.golden()
    case = KC.build("db1")
    voc = ORBVocabulary(KC.vocabulary(), ctx)
    for (a, b), want in list(zip(KC.score_pairs(case), G["db1_pair_score"]))[:3]:
        assert np.float64(voc.score(KC.bow_of(case, a), KC.bow_of(case, b))).view(np.uint64) == want.view(np.uint64)


def test_bow_transform_feeds_the_detection_on_the_device(ctx, batch):
    """planar_bow_transform_dev -> planar_kfdb_detect_dev on device pointers, nothing copied in between: equals the oracle chain (the oracle's BowVectors through the
    real reference's database)"""
    from planarslam_amd._lib import check, lib
    from planarslam_amd.bow import ORBVocabulary
    db, modes = batch
    m = modes[0]
    B = len(m["q_db"])
    voc = ORBVocabulary(KC.vocabulary(), ctx)
    desc = np.zeros((B, W, 32), np.uint8)
    nf = np.array([len(q["desc"]) for q in m["queries"]], np.int32)
    for b, q in enumerate(m["queries"]):
        desc[b, :nf[b]] = q["desc"]
    d = Device()
    view = d.database(db)
    d_desc, d_nf = d.up(desc), d.up(nf)
    d_word, d_weight, d_node = d.up(np.zeros((B, W), np.int32)), d.up(np.zeros((B, W))), d.up(np.zeros((B, W), np.int32))
    d_bw, d_bv, d_bn = d.up(np.zeros((B, W), np.int32)), d.up(np.zeros((B, W))), d.up(np.zeros(B, np.int32))
    d_qdb = d.up(m["q_db"])
    first = len(d.keep)
    cand0 = np.full((B, S), CAND_SENTINEL, np.int32)
    outs = [d.up(m["score_in"]), d.up(np.zeros((B, S), np.int32)), d.up(np.zeros(B, np.int32)), d.up(cand0), d.up(np.zeros(B, np.int32))]
    d.torch.cuda.synchronize()
    check(lib().planar_bow_transform_dev(voc.h, d_desc, d_nf, B, W, 4, d_word, d_weight, d_node, d_bw, d_bv, d_bn))
    check(lib().planar_kfdb_detect_dev(ctx.h, 0, C.byref(view), B, d_qdb, d_bn, d_bw, d_bv, W, None, None, *outs))
    ctx.sync()
    ref = m["ref"]
    np.testing.assert_array_equal(d.down(first - 2, np.zeros(B, np.int32)), m["n"])
    np.testing.assert_array_equal(d.down(first, m["score_in"]).view(np.uint32), ref["score"].view(np.uint32))
    np.testing.assert_array_equal(d.down(first + 1, np.zeros((B, S), np.int32)), ref["common"])
    np.testing.assert_array_equal(d.down(first + 2, np.zeros(B, np.int32)), ref["n_cand"])
    np.testing.assert_array_equal(d.down(first + 4, np.zeros(B, np.int32)), ref["n_scored"])
    cand = d.down(first + 3, cand0)
    for b in range(B):
        assert cand[b, :ref["n_cand"][b]].tolist() == ref["cand"][b, :ref["n_cand"][b]].tolist()


def test_limits_and_alignment_are_einval(ctx):
    from planarslam_amd import kfdb
    from planarslam_amd._lib import KFDB_MAX_KEYFRAMES, KFDB_MAX_WORDS, PlanarError, lib

    def database(S_, W_):
        return dict(n_kf=np.zeros(1, np.int32), present=np.zeros((1, S_), np.uint8), add_seq=np.zeros((1, S_), np.int32), bow_n=np.zeros((1, S_), np.int32),
                    bow_word=np.zeros((1, S_, W_), np.int32), bow_value=np.zeros((1, S_, W_)), covis=np.full((1, S_, 10), -1, np.int32))

    one = np.zeros(1, np.int32)
    for S_, W_, QW in ((KFDB_MAX_KEYFRAMES + 1, 8, 8), (8, KFDB_MAX_WORDS + 1, 8), (8, 8, KFDB_MAX_WORDS + 1)):
        with pytest.raises(PlanarError) as e:
            kfdb.detect(ctx, 0, database(S_, W_), one, one, np.zeros((1, QW), np.int32), np.zeros((1, QW)))
        assert e.value.code == -1
    kfdb.detect(ctx, 0, database(8, 8), one, one, np.zeros((1, 8), np.int32), np.zeros((1, 8)))      # within the limits: accepted
    # a bow_value that does not start on an 8-byte boundary
    v, keep = kfdb.kf_database(database(8, 8))
    raw = np.zeros(8 * 8 * 8 + 8, np.uint8)
    v.bow_value = raw.ctypes.data + 4
    out = [np.zeros((1, 8), np.float32), np.zeros((1, 8), np.int32), one.copy(), np.zeros((1, 8), np.int32), one.copy()]
    qw, qv = np.zeros((1, 8), np.int32), np.zeros((1, 8))
    args = [one.ctypes.data, one.ctypes.data, qw.ctypes.data, qv.ctypes.data, 8, None, None] + [a.ctypes.data for a in out]
    assert lib().planar_kfdb_detect(ctx.h, 0, C.byref(v), 1, *args) == -1
    assert lib().planar_kfdb_detect_dev(ctx.h, 0, C.byref(v), 1, *args) == -1
    assert b"8-byte" in lib().planar_last_error()
    with pytest.raises(PlanarError):                                                                   # loop mode without its two arrays
        kfdb.detect(ctx, 1, database(8, 8), one, one, np.zeros((1, 8), np.int32), np.zeros((1, 8)))
    wide = np.zeros((1, KFDB_MAX_WORDS + 1), np.int32)
    with pytest.raises(PlanarError):
        kfdb.bow_score(ctx, one, wide, wide.astype(np.float64), one, np.zeros((1, 8), np.int32), np.zeros((1, 8)))


def test_python_mirror_follows_the_reference_through_the_sequence(ctx):
    """planarslam_amd.kfdb.KeyFrameDatabase: add / erase / add again, then one query per call; slots are handed out in add() order, so they differ from the ids"""
    from planarslam_amd.kfdb import KeyFrameDatabase
    G = KH.golden()
    case = KC.build("db2")
    n = case["n_kf"]
    db = KeyFrameDatabase(ctx, kf_stride=32, word_stride=320)
    for op, j in case["ops"]:
        if op == 0:
            db.add(j, *case["kf_bow"][j], covisible=[int(k) for k in case["covis"][j] if k >= 0])
        else:
            db.erase(j)
    assert [db.slot[j] for j in range(n)] != list(range(n))
    members = {0: db.reloc_score, 1: db.loop_score}
    for q, query in enumerate(case["queries"]):
        bow = [(query["word"], query["value"])]
        if query["mode"] == 0:
            got = db.DetectRelocalizationCandidates(bow)[0]
        else:
            got = db.DetectLoopCandidates(bow, [np.nonzero(query["excluded"])[0].tolist()], [query["min_score"]])[0]
        assert got == G["db2_cand"][q, :G["db2_n_cand"][q]].tolist(), q
        by_id = np.array([members[query["mode"]][db.slot[j]] for j in range(n)], np.float32)
        assert by_id.view(np.uint32).tolist() == G["db2_score"][q, :n].view(np.uint32).tolist(), q
    db.clear()
    assert db.d["n_kf"][0] == 0 and not db.slot
