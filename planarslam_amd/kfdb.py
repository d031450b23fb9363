"""KeyFrameDatabase (src/KeyFrameDatabase.cc) on the device: thin mirrors of planar_kfdb_detect and planar_bow_score over dict-of-arrays databases, and a
`KeyFrameDatabase` class with the reference's add / erase / clear / DetectRelocalizationCandidates / DetectLoopCandidates that keeps the padded arrays.

A database dict holds the arrays of planar_kf_database for G databases: n_kf [G], present, add_seq, bow_n [G, S], bow_word, bow_value [G, S, W], covis [G, S, 10]."""
import ctypes as C

import numpy as np

from ._lib import KFDB_MAX_KEYFRAMES, KFDB_MAX_WORDS, Context, KfDatabase, check, lib

NCOVIS = 10
_FIELDS = (("n_kf", np.int32), ("present", np.uint8), ("add_seq", np.int32), ("bow_n", np.int32), ("bow_word", np.int32), ("bow_value", np.float64), ("covis", np.int32))


def kf_database(d: dict):
    """dict -> (planar_kf_database, keepalive)"""
    v, keep = KfDatabase(), {}
    v.kf_stride, v.word_stride = d["bow_word"].shape[-2:]
    for name, dt in _FIELDS:
        keep[name] = np.ascontiguousarray(d[name], dt)
        setattr(v, name, keep[name].ctypes.data)
    return v, keep


def detect(ctx: Context, mode: int, db: dict, q_db, q_bow_n, q_bow_word, q_bow_value, excluded=None, min_score=None, score=None, cand=None):
    """mode 0: DetectRelocalizationCandidates, 1: DetectLoopCandidates, for B queries -> dict(score [B, S] float32 (`score` on entry: mRelocScore / mLoopScore, zeros if
    None), common_words [B, S], n_cand [B], cand [B, S] (rows beyond n_cand keep what `cand` held, -1 if None), n_scored [B])"""
    v, keep = kf_database(db)
    S = v.kf_stride
    qd = np.ascontiguousarray(q_db, np.int32); qn = np.ascontiguousarray(q_bow_n, np.int32)
    qw = np.ascontiguousarray(q_bow_word, np.int32); qv = np.ascontiguousarray(q_bow_value, np.float64)
    B = len(qd)
    ex = None if excluded is None else np.ascontiguousarray(excluded, np.uint8)
    ms = None if min_score is None else np.ascontiguousarray(min_score, np.float32)
    out = dict(score=np.zeros((B, S), np.float32) if score is None else np.array(score, np.float32), common_words=np.zeros((B, S), np.int32), n_cand=np.zeros(B, np.int32),
               cand=np.full((B, S), -1, np.int32) if cand is None else np.array(cand, np.int32), n_scored=np.zeros(B, np.int32))
    p = lambda a: None if a is None else a.ctypes.data
    check(lib().planar_kfdb_detect(ctx.h, int(mode), C.byref(v), B, p(qd), p(qn), p(qw), p(qv), qw.shape[-1], p(ex), p(ms), p(out["score"]), p(out["common_words"]),
                                   p(out["n_cand"]), p(out["cand"]), p(out["n_scored"])))
    return out


def bow_score(ctx: Context, a_n, a_word, a_value, b_n, b_word, b_value):
    """L1Scoring::score for P pairs of padded BowVectors -> [P] float64"""
    an = np.ascontiguousarray(a_n, np.int32); aw = np.ascontiguousarray(a_word, np.int32); av = np.ascontiguousarray(a_value, np.float64)
    bn = np.ascontiguousarray(b_n, np.int32); bw = np.ascontiguousarray(b_word, np.int32); bv = np.ascontiguousarray(b_value, np.float64)
    out = np.zeros(len(an), np.float64)
    check(lib().planar_bow_score(ctx.h, len(an), an.ctypes.data, aw.ctypes.data, av.ctypes.data, aw.shape[-1], bn.ctypes.data, bw.ctypes.data, bv.ctypes.data, bw.shape[-1],
                                 out.ctypes.data))
    return out


def pad_bow(vectors, stride=None):
    """[(word, value)] -> (n [P], word [P, stride], value [P, stride])"""
    n = np.array([len(w) for w, _ in vectors], np.int32)
    stride = max(int(n.max(initial=0)), 1) if stride is None else stride
    w = np.zeros((len(vectors), stride), np.int32); v = np.zeros((len(vectors), stride))
    for i, (a, b) in enumerate(vectors):
        w[i, :n[i]] = a; v[i, :n[i]] = b
    return n, w, v


class KeyFrameDatabase:
    """One database.  Key frames are named by the caller's ids (KeyFrame::mnId); a key frame keeps its slot when it is erased and added again.  The score members
    (mRelocScore, mLoopScore) live here and start at 0.  A batched query call hands every query the members as they stand on entry; afterwards the members hold what
    the queries assigned, the later query of the batch winning - for one query per call that is the reference's sequence."""

    def __init__(self, ctx: Context | None = None, kf_stride: int = 256, word_stride: int = 1024):
        if not (1 <= kf_stride <= KFDB_MAX_KEYFRAMES and 1 <= word_stride <= KFDB_MAX_WORDS):
            raise ValueError("kf_stride / word_stride beyond PLANAR_KFDB_MAX_KEYFRAMES / PLANAR_KFDB_MAX_WORDS")
        self.ctx = ctx or Context(0)
        self.kf_stride, self.word_stride = kf_stride, word_stride
        self.clear()

    def clear(self):
        S, W = self.kf_stride, self.word_stride
        self.slot, self.ids, self.covis_ids, self.seq = {}, [], {}, 0
        self.d = dict(n_kf=np.zeros(1, np.int32), present=np.zeros((1, S), np.uint8), add_seq=np.zeros((1, S), np.int32), bow_n=np.zeros((1, S), np.int32),
                      bow_word=np.zeros((1, S, W), np.int32), bow_value=np.zeros((1, S, W)), covis=np.full((1, S, NCOVIS), -1, np.int32))
        self.reloc_score = np.zeros(S, np.float32)
        self.loop_score = np.zeros(S, np.float32)

    def add(self, kf_id, bow_word, bow_value, covisible=None):
        """KeyFrameDatabase::add(pKF); covisible: the ids GetBestCovisibilityKeyFrames(10) returns (also settable later, set_covisibility)"""
        j = self.slot.get(kf_id)
        if j is None:
            if len(self.ids) >= self.kf_stride:
                raise ValueError("more key frames than kf_stride")
            j = self.slot[kf_id] = len(self.ids)
            self.ids.append(kf_id)
            self.d["n_kf"][0] = len(self.ids)
        elif self.d["present"][0, j]:
            raise ValueError("key frame is in the database already")
        n = len(bow_word)
        if n > self.word_stride:
            raise ValueError("more words than word_stride")
        self.d["bow_n"][0, j] = n
        self.d["bow_word"][0, j, :n] = bow_word; self.d["bow_value"][0, j, :n] = bow_value
        self.d["present"][0, j] = 1; self.d["add_seq"][0, j] = self.seq
        self.seq += 1
        if covisible is not None:
            self.set_covisibility(kf_id, covisible)

    def set_covisibility(self, kf_id, covisible):
        self.covis_ids[kf_id] = list(covisible)[:NCOVIS]

    def erase(self, kf_id):
        self.d["present"][0, self.slot[kf_id]] = 0

    def _refresh_covis(self):
        self.d["covis"][:] = -1
        for kf_id, ids in self.covis_ids.items():
            if kf_id in self.slot:
                self.d["covis"][0, self.slot[kf_id], :len(ids)] = [self.slot.get(i, -1) for i in ids]

    def _detect(self, mode, bows, members, excluded_ids=None, min_score=None):
        self._refresh_covis()
        n, w, v = pad_bow(bows)
        B = len(bows)
        ex = None
        if mode == 1:
            ex = np.zeros((B, self.kf_stride), np.uint8)
            for b, ids in enumerate(excluded_ids):
                for i in ids:
                    if i in self.slot:
                        ex[b, self.slot[i]] = 1
        r = detect(self.ctx, mode, self.d, np.zeros(B, np.int32), n, w, v, ex, min_score, score=np.repeat(members[None], B, 0))
        for b in range(B):
            assigned = r["common_words"][b] > int(np.float32(r["common_words"][b].max()) * np.float32(0.8))
            members[assigned] = r["score"][b][assigned]
        return [[self.ids[j] for j in r["cand"][b, :r["n_cand"][b]]] for b in range(B)]

    def DetectRelocalizationCandidates(self, bows):
        """bows: [(bow_word, bow_value)] of B frames -> B lists of key-frame ids, in the reference's order"""
        return self._detect(0, bows, self.reloc_score)

    def DetectLoopCandidates(self, bows, connected, min_score):
        """bows of B query key frames, connected: B collections of ids (GetConnectedKeyFrames), min_score [B] -> B lists of key-frame ids"""
        return self._detect(1, bows, self.loop_score, connected, np.asarray(min_score, np.float32))
