"""Time planar_optimize_sim3_dev against the single-thread host build of the same source (planarslam_amd/csrc/sim3_arith.h through tests/host_shim/sim3_opt_host.cpp,
g++ -O3): B = 1 and B = 64 pairs of about `--matches` correspondences each.  Events on the context's stream, warm-up, repeated launches, the median; S12 and match12
are restored before every launch (outside the timed span).  The batch tiles `--distinct` generated pairs.  Each B is timed in a child process of its own under a time
limit, so a fault or a hang in one ends that step alone and nothing more is started.  Prints one JSON line per B.
    python tools/sim3_opt_bench.py [--B 64] [--matches 150] [--reps 20] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))


def problem(B, distinct, matches):
    import sim3_opt_cases as SC
    from loop_match_bench import tile, tile_dict
    D = min(B, distinct)
    stride = -(-int(matches * 1.3) // 64) * 64
    case = SC.opt_case(B=D, N=matches, stride=stride, seed=801, scales=(1.0, 0.9, 1.1), fix_scale=1, outliers=0.15)
    out = dict(case, S12=tile(case["S12"], B), match12=tile(case["match12"], B))
    out["kf1"], out["kf2"] = tile_dict(case["kf1"], B, skip=("scale_factors",)), tile_dict(case["kf2"], B, skip=("scale_factors",))
    return out


def one(B, a):
    import torch
    import loop_match_cases as LC
    import sim3_opt_cases as SC
    from planarslam_amd._lib import Context, check, lib
    case = problem(B, a.distinct, a.matches)
    ctx = Context(0)
    stream = torch.cuda.ExternalStream(lib().planar_ctx_get_stream(ctx.h))
    d = LC.Device()
    args, keep, first = SC.dev_args(d, case)
    likes = [np.zeros((B, 8), np.float64), np.zeros(case["match12"].shape, np.int32), np.zeros(B, np.int32), np.zeros((B, 2), np.int32)]
    inout = [d.keep[first + i] for i in range(2)]
    pristine = [t.clone() for t in inout]
    fn = lib().planar_optimize_sim3_dev
    torch.cuda.synchronize()
    for _ in range(a.warmup):
        for t, p in zip(inout, pristine):
            t.copy_(p)
        torch.cuda.synchronize()
        check(fn(ctx.h, *args))
    ctx.sync()
    ms = []
    for _ in range(a.reps):
        for t, p in zip(inout, pristine):
            t.copy_(p)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); check(fn(ctx.h, *args)); e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    S12, m, nin, its = [d.down(first + i, like) for i, like in enumerate(likes)]
    L = SC.load_host("-O3")
    host_ms = []
    for _ in range(3):
        t = time.perf_counter()
        h = SC.host_run(L, case, events=False)
        host_ms.append((time.perf_counter() - t) * 1e3)
    return dict(what="planar_optimize_sim3_dev", B=B, matches=a.matches, correspondences_mean=float(np.mean([(r >= 0).sum() for r in case["match12"]])),
                distinct_problems=min(B, a.distinct), inliers=int(nin.sum()), flags_equal_host_vs_device=bool(np.array_equal(h[0], m) and np.array_equal(h[1], nin)),
                lm_iters_mean=float(its.sum(1).mean()), reps=a.reps, device_ms_median=float(np.median(ms)),
                device_ms_min=float(min(ms)), device_ms_max=float(max(ms)), host_1_thread_ms_median=float(np.median(host_ms)),
                s12_difference_host_vs_device=SC.s12_difference(h[2], S12), host_note="sim3_arith.h under g++ -O3, one thread, called per pair through ctypes",
                gpu=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64); ap.add_argument("--matches", type=int, default=150); ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20); ap.add_argument("--warmup", type=int, default=3); ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=120, help="seconds per B"); ap.add_argument("--one", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one, a)))
        return 0
    lines = []
    for B in (1, a.B):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", str(B), "--matches", str(a.matches), "--distinct", str(a.distinct),
               "--reps", str(a.reps), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            print(f"B={B}: exit status {r.returncode}; nothing more is started", file=sys.stderr)
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
