"""Time the four loop-closing matchers' _dev entry points against the sequential restatement tests/host_shim/loop_match_host.cpp (one host thread, -O3): B = 1 and a batch
of a few hundred problems at ~1000 features per key frame, and for the two Scw entries 6000 points per problem.  Events on the context's stream, warm-up, repeated launches,
the median; the in/out arrays are restored before every launch (outside the timed span).  The batch tiles `--distinct` generated problems.  Each (entry, B) is timed in
a child process of its own under a time limit, so a fault or a hang in one ends that step alone and nothing more is started.  Prints one JSON line per (entry, B).
    python tools/loop_match_bench.py [--B 256] [--features 1000] [--points 6000] [--reps 20] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
ENTRIES = ("bow", "sim3", "proj", "fuse")


def tile(a, B):
    """the first axis repeated up to B problems"""
    reps = -(-B // a.shape[0])
    return np.ascontiguousarray(np.concatenate([a] * reps)[:B])


def tile_dict(d, B, skip=()):
    return {k: (tile(v, B) if isinstance(v, np.ndarray) and v.ndim >= 1 and k not in skip else v) for k, v in d.items()}


def problem(entry, B, distinct, features, points):
    import loop_match_cases as LC
    D = min(B, distinct)
    stride = -(-int(features * 1.02) // 64) * 64
    if entry == "bow":
        case = LC.bow_case(B=D, N=int(features * 0.8), stride=stride, seed=601, ns=[int(features * 0.8)] * D)
        return tile_dict(case, B)
    if entry == "sim3":
        case = LC.sim3_case(B=D, N=int(features * 0.8), stride=stride, seed=602, ns=[int(features * 0.8)] * D)
        out = tile_dict(case, B)
        out["kf1"], out["kf2"] = tile_dict(case["kf1"], B, skip=("scale_factors",)), tile_dict(case["kf2"], B, skip=("scale_factors",))
        return out
    case = LC.scw_case(B=D, N=features, NP=points, stride=stride, seed=603, ns=[features] * D, nps=[points] * D)
    out = tile_dict(case, B)
    out["kf"], out["pts"] = tile_dict(case["kf"], B, skip=("scale_factors",)), tile_dict(case["pts"], B)
    return out


def one(entry, B, a):
    import torch
    import loop_match_cases as LC
    from planarslam_amd._lib import Context, check, lib
    case = problem(entry, B, a.distinct, a.features, a.points)
    ctx = Context(0)
    stream = torch.cuda.ExternalStream(lib().planar_ctx_get_stream(ctx.h))
    d = LC.Device()
    L = LC.load_host("-O3")
    if entry == "bow":
        m0 = np.full(case["node1"].shape, -1, np.int32)
        fn, args, first, likes = LC.bow_dev_args(d, case, 0.75, True, m0)
        host = lambda: LC.host_bow(L, case, 0.75, True)
        accepted = lambda h: int(h[1].sum())
        same = lambda h, g: np.array_equal(h[0], g[0]) and np.array_equal(h[1], g[1])
    elif entry == "sim3":
        fn = lib().planar_search_by_sim3_dev
        args, keep, first = LC.sim3_dev_args(d, case, 7.5, case["match12"])
        likes = [np.zeros(case["match12"].shape, np.int32), np.zeros(B, np.int32)]
        host = lambda: LC.host_sim3(L, case, 7.5, report=False)
        accepted = lambda h: int(h[1].sum())
        same = lambda h, g: np.array_equal(h[0], g[0]) and np.array_equal(h[1], g[1])
    elif entry == "proj":
        m0 = np.full(case["kf"]["keys_un"].shape, -1, np.int32)
        fn, args, first, likes = LC.proj_dev_args(d, case, 10, m0)
        host = lambda: LC.host_projection_scw(L, case, 10)
        accepted = lambda h: int(h[1].sum())
        same = lambda h, g: np.array_equal(h[0], g[0]) and np.array_equal(h[1], g[1])
    else:
        f0 = np.full(case["usable_b"].shape, -9, np.int32)
        fn, args, first, likes = LC.fuse_dev_args(d, case, 4.0, f0, f0)
        host = lambda: LC.host_fuse_scw(L, case, 4.0)
        accepted = lambda h: int(h[2].sum())
        same = lambda h, g: all(np.array_equal(h[i], g[i]) for i in range(3))
    inout = [d.keep[first + i] for i in range(len(likes))]
    pristine = [t.clone() for t in inout]

    def launch():
        check(fn(ctx.h, *args))
    torch.cuda.synchronize()
    for _ in range(a.warmup):
        launch()
    ctx.sync()
    ms = []
    for _ in range(a.reps):
        for t, p in zip(inout, pristine):
            t.copy_(p)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); launch(); e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    got = [d.down(first + i, like) for i, like in enumerate(likes)]
    host_ms = []
    for _ in range(3):
        t = time.perf_counter()
        h = host()
        host_ms.append((time.perf_counter() - t) * 1e3)
    assert same(h, got), "the device result differs from the restatement"
    return dict(what="planar_" + {"bow": "search_by_bow_kf", "sim3": "search_by_sim3", "proj": "search_by_projection_sim3", "fuse": "fuse_sim3"}[entry] + "_dev", B=B,
                features=a.features, points=a.points if entry in ("proj", "fuse") else None, distinct_problems=min(B, a.distinct), accepted=accepted(h), reps=a.reps,
                device_ms_median=float(np.median(ms)), device_ms_min=float(min(ms)), device_ms_max=float(max(ms)), host_1_thread_ms_median=float(np.median(host_ms)),
                host_note="the -O3 restatement called per problem through ctypes, its grid built per call", gpu=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256); ap.add_argument("--features", type=int, default=1000); ap.add_argument("--points", type=int, default=6000)
    ap.add_argument("--distinct", type=int, default=8); ap.add_argument("--reps", type=int, default=20); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None); ap.add_argument("--limit", type=int, default=150, help="seconds per (entry, B) step")
    ap.add_argument("--one", nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one[0], int(a.one[1]), a)))
        return 0
    lines = []
    for entry in ENTRIES:
        for B in (1, a.B):
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", entry, str(B), "--features", str(a.features), "--points", str(a.points),
                   "--distinct", str(a.distinct), "--reps", str(a.reps), "--warmup", str(a.warmup)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:
                print(f"{entry} B={B}: exit status {r.returncode}; nothing more is started", file=sys.stderr)
                return r.returncode
            line = r.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
