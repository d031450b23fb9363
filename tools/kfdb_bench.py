"""Time planar_kfdb_detect_dev against the host restatement tests/host_shim/kfdb_host.cpp (one thread, -O3): 256 queries x 256 key frames x ~1000 words by default,
in both modes; events on the context's stream, warm-up, repeated launches, the median.  Prints one JSON line per mode.  Makes no statement about B = 1.
    python tools/kfdb_bench.py [--B 256] [--kf 256] [--words 1000] [--reps 20]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def synthetic(B, n_kf, words, seed=5):
    """one database of n_kf key frames whose word sets slide over a word range (neighbours overlap), B queries that are noisy copies of key frames"""
    rng = np.random.default_rng(seed)
    W = int(words * 1.25)
    step = max(words // 6, 1)
    pool = np.sort(rng.choice(10 ** 6, n_kf * step + 2 * words, replace=False)).astype(np.int32)
    db = dict(n_kf=np.array([n_kf], np.int32), present=np.ones((1, n_kf), np.uint8), add_seq=rng.permutation(n_kf).astype(np.int32)[None],
              bow_n=np.zeros((1, n_kf), np.int32), bow_word=np.zeros((1, n_kf, W), np.int32), bow_value=np.zeros((1, n_kf, W)), covis=np.full((1, n_kf, 10), -1, np.int32))

    def vector(start, n):
        w = np.sort(rng.choice(pool[start:start + 2 * words], n, replace=False))
        v = rng.uniform(0.5, 9.0, n)
        return w, v / v.sum()
    for j in range(n_kf):
        n = int(rng.integers(int(words * 0.8), W))
        w, v = vector(j * step, n)
        db["bow_n"][0, j] = n; db["bow_word"][0, j, :n] = w; db["bow_value"][0, j, :n] = v
        near = [k for k in (j - 1, j + 1, j - 2, j + 2, j - 3, j + 3, j - 4, j + 4, j - 5, j + 5) if 0 <= k < n_kf]
        db["covis"][0, j, :len(near)] = near
    qn = np.zeros(B, np.int32); qw = np.zeros((B, W), np.int32); qv = np.zeros((B, W))
    ex = np.zeros((B, n_kf), np.uint8)
    for b in range(B):
        j = int(rng.integers(0, n_kf))
        n = int(rng.integers(int(words * 0.8), W))
        w, v = vector(j * step, n)
        qn[b] = n; qw[b, :n] = w; qv[b, :n] = v
        ex[b, max(j - 1, 0):j + 2] = 1
    return db, qn, qw, qv, ex, np.full(B, 0.05, np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256); ap.add_argument("--kf", type=int, default=256); ap.add_argument("--words", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20); ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    import kfdb_host as KH
    from planarslam_amd import kfdb
    from planarslam_amd._lib import Context, check, lib
    L = KH.load_host("-O3")
    db, qn, qw, qv, ex, ms_in = synthetic(a.B, a.kf, a.words)
    ctx = Context(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.ExternalStream(lib().planar_ctx_get_stream(ctx.h))
    keep = []

    def up(x):
        keep.append(torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev))
        return keep[-1].data_ptr()
    view, arrays = kfdb.kf_database(db)
    for name, arr in arrays.items():
        setattr(view, name, up(arr))
    ins = [up(np.zeros(a.B, np.int32)), up(qn), up(qw), up(qv)]
    d_ex, d_ms = up(ex), up(ms_in)
    score = torch.zeros(a.B * a.kf, dtype=torch.float32, device=dev)
    common, cand = (torch.zeros(a.B * a.kf, dtype=torch.int32, device=dev) for _ in range(2))
    n_cand, n_scored = (torch.zeros(a.B, dtype=torch.int32, device=dev) for _ in range(2))
    one = {k: v[0] for k, v in db.items()}
    for mode in (0, 1):
        def launch():
            check(lib().planar_kfdb_detect_dev(ctx.h, mode, C.byref(view), a.B, *ins, qw.shape[1], d_ex if mode else None, d_ms if mode else None, score.data_ptr(),
                                               common.data_ptr(), n_cand.data_ptr(), cand.data_ptr(), n_scored.data_ptr()))
        torch.cuda.synchronize()
        for _ in range(a.warmup):
            score.zero_(); launch()
        ctx.sync()
        ms = []
        for _ in range(a.reps):
            score.zero_()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream); launch(); e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        dev_n, dev_scored = n_cand.cpu().numpy(), n_scored.cpu().numpy()
        host_ms = []
        for _ in range(3):
            t = time.perf_counter()
            rows = [KH.host_detect(L, one, mode, qw[b, :qn[b]], qv[b, :qn[b]], ex[b] if mode else None, ms_in[b], np.zeros(a.kf, np.float32), report=False) for b in range(a.B)]
            host_ms.append((time.perf_counter() - t) * 1e3)
        assert [r["n_cand"] for r in rows] == dev_n.tolist() and [r["n_scored"] for r in rows] == dev_scored.tolist()
        print(json.dumps(dict(what="planar_kfdb_detect_dev", mode=mode, B=a.B, key_frames=a.kf, words=a.words, scored_pairs=int(dev_scored.sum()), candidates=int(dev_n.sum()),
                              reps=a.reps, device_ms_median=float(np.median(ms)), device_ms_min=float(min(ms)), device_ms_max=float(max(ms)),
                              host_1_thread_ms_median=float(np.median(host_ms)), host_note="includes building the inverted file per query and the ctypes call",
                              gpu=torch.cuda.get_device_name(0))))


if __name__ == "__main__":
    main()
